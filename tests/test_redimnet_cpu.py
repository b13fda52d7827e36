"""ReDimNetB2 without a GPU: the parameter table (arch.py's and the library's) against the fixtures'
names and shapes, the host-side surface (registry, defaults, refusals, the C ABI's create / refuse
matrix), the multiply-accumulate count, the synthetic rule for inputs_weights, and the torch
restatement tests/redimnet_ref.py against the fixtures made from the reference module
(tests/golden/make_redimnet_golden.py): in float64 it is the reference's float64 run to 1e-9, in
float32 it stays within 2e-5 of it (the reference's own float32 run is within 4.6e-6 on these
cases; 4x for other hosts' conv kernels)."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import redimnet_ref  # noqa: E402
from redimnet_cases import ARCH, FIXTURES, IDS, SEED, TAPS, load_case  # noqa: E402
from wespeaker_hubert_amd import _lib  # noqa: E402
from wespeaker_hubert_amd import arch as A  # noqa: E402
from wespeaker_hubert_amd.speaker_model import HipSpeakerModel, get_speaker_model  # noqa: E402
from wespeaker_hubert_amd.synthetic import synth_param  # noqa: E402

COUNT = 548
WANT = {"redimnet_b2_t200", "redimnet_b3_t2", "redimnet_b1_t30", "redimnet_b1_t37_e256_2emb", "redimnet_b2_t301",
        "redimnet_b3_t64_mixed"}


def test_the_six_fixtures_exist():
    assert set(IDS) == WANT
    for p in FIXTURES:
        assert os.path.getsize(p) < 64 * 1024
        assert int(np.load(p)["weight_seed"]) == SEED


def test_make_spec_defaults_and_refusals():
    s = A.make_spec(ARCH)
    assert (s.feat_dim, s.embed_dim, s.pooling_func, s.two_emb_layer, s.family) == (72, 192, "ASTP", False, "redimnet")
    assert A.make_spec(ARCH, feat_dim=72, embed_dim=256, two_emb_layer=True).two_emb_layer
    for other in ("ReDimNetB0", "ReDimNetB1", "ReDimNetB3", "ReDimNetB4", "ReDimNetB5", "ReDimNetB6"):
        with pytest.raises(NotImplementedError, match="ReDimNetB2"):
            A.make_spec(other)
        with pytest.raises(NotImplementedError, match="ReDimNetB2"):
            get_speaker_model(other)
    with pytest.raises(ValueError, match="feat_dim"):
        A.make_spec(ARCH, feat_dim=80)
    with pytest.raises(NotImplementedError, match="ASTP"):
        A.make_spec(ARCH, pooling_func="TSTP")
    with pytest.raises(TypeError, match="emb_bn"):
        A.make_spec(ARCH, emb_bn=False)
    with pytest.raises(KeyError):
        A.make_spec("ReDimNetB9")
    with pytest.raises(KeyError):
        get_speaker_model("ReDimNetB9")


def test_registry():
    m = get_speaker_model(ARCH)(feat_dim=72, embed_dim=192)
    assert isinstance(m, HipSpeakerModel) and m.spec.family == "redimnet" and not m.supports_segments
    assert len(m.state_dict_layout()) == COUNT
    assert len(get_speaker_model(ARCH)(two_emb_layer=True).state_dict_layout()) == COUNT + 5


@pytest.mark.parametrize("path", FIXTURES, ids=IDS)
def test_param_layout_matches_reference(path):
    z, spec, plist, _, _ = load_case(path)
    assert A.param_list(spec) == plist and spec.family == "redimnet"
    assert [n for n, _ in plist] == [str(n) for n in z["param_names"]]
    assert [tuple(s) for _, s in plist] == [tuple(int(s) for s in str(v).split(",") if s) for v in z["param_shapes"]]
    assert len(plist) == COUNT + 5 * spec.two_emb_layer


def _library_table(arch, feat_dim, embed_dim, two_emb):
    lib = _lib.load()
    h = ctypes.c_void_p()
    assert lib.wsp_model_create(arch.encode(), feat_dim, embed_dim, 0, int(two_emb), ctypes.byref(h)) == 0, \
        lib.wsp_last_error()
    try:
        name, ndim, shape = ctypes.c_char_p(), ctypes.c_int(), (ctypes.c_int64 * 4)()
        out = []
        for i in range(lib.wsp_model_num_params(h)):
            assert lib.wsp_model_param_info(h, i, ctypes.byref(name), ctypes.byref(ndim), shape) == 0
            out.append((name.value.decode(), tuple(shape[d] for d in range(ndim.value))))
        return out
    finally:
        lib.wsp_model_destroy(h)


@pytest.mark.parametrize("two_emb", (False, True))
def test_library_table_matches_arch(two_emb):
    want = A.param_list(A.make_spec(ARCH, embed_dim=256, two_emb_layer=two_emb))
    assert _library_table(ARCH, 72, 256, two_emb) == [(n, tuple(s)) for n, s in want]


def test_library_create_and_refuse_matrix():
    lib = _lib.load()
    h = ctypes.c_void_p()
    for other in ("ReDimNetB0", "ReDimNetB1", "ReDimNetB3", "ReDimNetB4", "ReDimNetB5", "ReDimNetB6", "ReDimNetB9",
                  "ReDimNet", "ReDimNetB2_x"):
        assert lib.wsp_model_create(other.encode(), 72, 192, 0, 0, ctypes.byref(h)) != 0
        assert b"unsupported arch" in lib.wsp_last_error()
    assert lib.wsp_model_create(b"ReDimNetB2", 80, 192, 0, 0, ctypes.byref(h)) != 0
    assert b"feat_dim 72" in lib.wsp_last_error()
    assert lib.wsp_model_create(b"ReDimNetB2", 72, 0, 0, 0, ctypes.byref(h)) != 0
    assert b"embed_dim" in lib.wsp_last_error()
    assert lib.wsp_model_create(b"ReDimNetB2", 72, 192, 1, 0, ctypes.byref(h)) != 0
    assert b"emb_bn" in lib.wsp_last_error()
    for two in (0, 1):
        assert lib.wsp_model_create(b"ReDimNetB2", 72, 192, 0, two, ctypes.byref(h)) == 0, lib.wsp_last_error()
        try:
            assert lib.wsp_model_num_params(h) == COUNT + 5 * two
            b = ctypes.c_size_t()
            # seven kept stage outputs and a ping-pong pair of [B * T][1152] floats, the narrow 1-D buffers on top
            assert lib.wsp_model_workspace_bytes(h, 2, 200, ctypes.byref(b)) == 0, lib.wsp_last_error()
            assert 9 * 400 * 1152 * 4 < b.value < 12 * 400 * 1152 * 4
        finally:
            lib.wsp_model_destroy(h)


def test_inputs_weights_draw_unit_normal_and_nothing_else_changes():
    w = synth_param(SEED, "backbone.inputs_weights.6", (1, 7, 1152, 1))
    assert w.dtype == np.float32 and abs(float(w.std()) - 1.0) < 0.05 and abs(float(w.mean())) < 0.05
    # the fan-in rule an unrelated name of the same shape still gets
    v = synth_param(SEED, "backbone.other_weights.6", (1, 7, 1152, 1))
    assert float(v.std()) < 0.02


def test_gflop_count():
    """2 x MACs from the parameter table alone (every conv / linear weight's element count times the
    frames it is applied at; a 2-D weight of a (c, F) stage is applied at F positions per frame) plus
    attention's two T x T products, against arch.redimnet_gflop_per_utt."""
    spec, T = A.make_spec(ARCH), 200
    macs = 0
    F_of = {f"backbone.stage{i}": d[4] for i, d in enumerate(A.redimnet_stage_dims(ARCH))}
    for name, shape in A.redimnet_params(spec):
        if not name.endswith(".weight") or len(shape) < 2:
            continue
        n = int(np.prod(shape))
        if len(shape) == 4:
            F = 72 if "stem" in name else F_of[name[:15]]
            macs += T * F * n
        elif name.startswith("pool.linear1"):
            macs += T * 128 * 1152 + 128 * 2 * 1152  # the context columns once per utterance
        elif name.startswith("seg_"):
            macs += n
        else:
            macs += T * n
    macs += sum(2 * T * T * d[6] for d in A.redimnet_stage_dims(ARCH))
    assert A.redimnet_gflop_per_utt(spec, T) == pytest.approx(2.0 * macs / 1e9, rel=1e-12)
    # the T^2 term is there
    g = A.redimnet_gflop_per_utt
    assert g(spec, 400) - 2 * g(spec, 200) + g(spec, 0) == pytest.approx(2.0 * 2 * 200 * 200 * 2 * (3 * 96 + 2 * 144 + 288) / 1e9, rel=1e-9)


_RUNS = {}


def _run(path):
    """the restatement in float64 (with taps) and float32, once per fixture"""
    if path not in _RUNS:
        z, _, _, sd, x = load_case(path)
        taps = {}
        e64 = redimnet_ref.forward(x, sd, taps=taps).numpy()
        e32 = redimnet_ref.forward(x, sd, dtype=torch.float32).numpy()
        _RUNS[path] = (z, e64, e32, taps)
    return _RUNS[path]


@pytest.mark.parametrize("path", FIXTURES, ids=IDS)
def test_ref_float64_equals_the_reference(path):
    z, e64, _, taps = _run(path)
    assert e64.dtype == np.float64 and e64.shape == z["embed64"].shape
    assert np.abs(e64 - z["embed64"]).max() < 1e-9
    for t in TAPS:
        for k in ("sum_" + t, "abs_" + t):
            assert abs(taps[k] - float(z[k])) <= 1e-9 * abs(float(z[k])), k
    # and the reference's own float32 run is as close to it as the bars assume
    assert np.abs(z["embed"].astype(np.float64) - z["embed64"]).max() <= 4.6e-6


@pytest.mark.parametrize("path", FIXTURES, ids=IDS)
def test_ref_float32_stays_near_float64(path):
    z, _, e32, _ = _run(path)
    d = np.abs(e32.astype(np.float64) - z["embed64"]).max()
    print(f"float32 restatement vs embed64: {d:.3e} (bar 2e-5)")
    assert d < 2e-5


def test_zeroing_the_input_weights_moves_the_embedding():
    """N(0, 1) input weights carry weight: with all of them zero (uniform softmax) the embedding of
    the T = 30 case moves by O(1), so a wrong softmax axis cannot hide."""
    z, _, _, sd, x = load_case([p for p in FIXTURES if p.endswith("redimnet_b1_t30.npz")][0])
    flat = {k: (np.zeros_like(v) if "inputs_weights" in k else v) for k, v in sd.items()}
    d = np.abs(redimnet_ref.forward(x, flat).numpy() - z["embed64"]).max()
    assert d > 0.5, d
