"""The host-only contract of the model handles (no GPU): every option default, alias,
refusal and workspace size equals tests/golden/host_contract.json, which
tests/golden/make_host_contract.py recorded from the library before the host runtime was
split by architecture; and the library's parameter tables equal arch.param_list."""
import ctypes
import importlib.util
import json
import os

import pytest

from wespeaker_hubert_amd import _lib
from wespeaker_hubert_amd import arch as A

GOLDEN = os.path.join(os.path.dirname(__file__), "golden")


def _generator():
    spec = importlib.util.spec_from_file_location("make_host_contract", os.path.join(GOLDEN, "make_host_contract.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.fixture(scope="module")
def recorded():
    with open(os.path.join(GOLDEN, "host_contract.json")) as f:
        want = json.load(f)
    got = json.loads(json.dumps(_generator().collect(_lib.load())))  # tuples / int keys as JSON has them
    return want, got


def test_every_handle_is_recorded(recorded):
    want, got = recorded
    assert sorted(want) == sorted(got) == sorted(_generator().HANDLES) and len(want) == 11


@pytest.mark.parametrize("name", sorted(_generator().HANDLES))
def test_options_and_workspace_equal_the_recorded_contract(recorded, name):
    want, got = recorded
    for section in sorted(set(want[name]) | set(got[name])):
        assert got[name][section] == want[name][section], (name, section)


def _library_params(arch, feat_dim, embed_dim, emb_bn=0, two_emb=0, in_planes=None):
    lib = _lib.load()
    h = ctypes.c_void_p()
    assert lib.wsp_model_create(arch.encode(), feat_dim, embed_dim, emb_bn, two_emb, ctypes.byref(h)) == 0
    try:
        if in_planes is not None:
            assert lib.wsp_model_set_option(h, b"in_planes", in_planes) == 0
        name, nd, shp = ctypes.c_char_p(), ctypes.c_int(), (ctypes.c_int64 * 4)()
        out = []
        for i in range(lib.wsp_model_num_params(h)):
            assert lib.wsp_model_param_info(h, i, ctypes.byref(name), ctypes.byref(nd), shp) == 0
            out.append((name.value.decode(), tuple(shp[d] for d in range(nd.value))))
        return out
    finally:
        lib.wsp_model_destroy(h)


@pytest.mark.parametrize("arch", sorted(A.ECAPA_ARCHS))
@pytest.mark.parametrize("emb_bn", (False, True))
def test_ecapa_parameter_table(arch, emb_bn):
    spec = A.make_spec(arch, feat_dim=80, embed_dim=192, emb_bn=emb_bn)
    assert _library_params(arch, 80, 192, emb_bn=int(emb_bn)) == [(n, tuple(s)) for n, s in A.param_list(spec)]


@pytest.mark.parametrize("arch", sorted(A.RESNET_ARCHS))
@pytest.mark.parametrize("two_emb", (False, True))
def test_resnet_parameter_table(arch, two_emb):
    spec = A.make_spec(arch, feat_dim=80, embed_dim=256, two_emb_layer=two_emb)
    assert _library_params(arch, 80, 256, two_emb=int(two_emb)) == [(n, tuple(s)) for n, s in A.param_list(spec)]


@pytest.mark.parametrize("arch", sorted(A.SIMAM_ARCHS))
@pytest.mark.parametrize("in_planes", (32, 64))
def test_simam_parameter_table(arch, in_planes):
    spec = A.make_spec(arch, acoustic_dim=80, embed_dim=256, in_planes=in_planes)
    assert _library_params(arch, 80, 256, in_planes=in_planes) == [(n, tuple(s)) for n, s in A.param_list(spec)]


@pytest.mark.parametrize("arch", sorted(A.CAMPP_ARCHS))
@pytest.mark.parametrize("feat_dim,embed_dim", ((80, 192), (64, 512)))
def test_campplus_parameter_table(arch, feat_dim, embed_dim):
    spec = A.make_spec(arch, feat_dim=feat_dim, embed_dim=embed_dim)
    assert _library_params(arch, feat_dim, embed_dim) == [(n, tuple(s)) for n, s in A.param_list(spec)]
