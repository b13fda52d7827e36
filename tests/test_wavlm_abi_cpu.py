"""CPU-only checks of the WavLM_base handle through the C-ABI (host-only until finalize):
parameter layout, rejected sizes, and that HuBERT_base's layout is unchanged."""
import ctypes

from wespeaker_hubert_amd import _lib
from wespeaker_hubert_amd.arch import hubert_params, wavlm_params


def _layout(lib, h):
    name, ndim, shape = ctypes.c_char_p(), ctypes.c_int(), (ctypes.c_int64 * 4)()
    out = []
    for i in range(lib.wsp_model_num_params(h)):
        assert lib.wsp_model_param_info(h, i, ctypes.byref(name), ctypes.byref(ndim), shape) == 0
        out.append((name.value.decode(), tuple(shape[d] for d in range(ndim.value))))
    return out


def test_wavlm_handle_layout_matches_wavlm_params():
    lib = _lib.load()
    h = ctypes.c_void_p()
    assert lib.wsp_model_create(b"WavLM_base", 1, 768, 0, 0, ctypes.byref(h)) == 0
    try:
        assert _layout(lib, h) == [(n, tuple(s)) for n, s in wavlm_params()]
        assert lib.wsp_model_embed_dim(h) == 768 and lib.wsp_model_feat_dim(h) == 1
        t, b, bh, v = ctypes.c_int(), ctypes.c_size_t(), ctypes.c_size_t(), ctypes.c_int()
        assert lib.wsp_frontend_out_frames(h, 80000, ctypes.byref(t)) == 0 and t.value == 250
        assert lib.wsp_frontend_out_frames(h, 399, ctypes.byref(t)) == 0 and t.value == 2
        assert lib.wsp_frontend_workspace_bytes(h, 4, 16000, ctypes.byref(b)) == 0 and b.value > 0
        assert lib.wsp_model_workspace_bytes(h, 4, 100, ctypes.byref(b)) != 0  # not a backbone handle
        # the shared front-end options exist on the handle, with HuBERT's defaults
        for key, want in ((b"streams", 2), (b"attn_pipe", 1), (b"ln_fold", 0), (b"pos_conv", 1), (b"layer", -1)):
            assert lib.wsp_model_get_option(h, key, ctypes.byref(v)) == 0 and v.value == want, key
        assert lib.wsp_model_set_option(h, b"layer", 13) != 0
        assert lib.wsp_model_set_option(h, b"layer", 6) == 0
        for pipe in (0, 1):  # both attention kernels carry the bias
            assert lib.wsp_model_set_option(h, b"attn_pipe", pipe) == 0
        # the gate adds 12 floats per frame to HuBERT's workspace, nothing else
        hh = ctypes.c_void_p()
        assert lib.wsp_model_create(b"HuBERT_base", 1, 768, 0, 0, ctypes.byref(hh)) == 0
        try:
            for key in (b"streams",):
                assert lib.wsp_model_set_option(h, key, 1) == 0 and lib.wsp_model_set_option(hh, key, 1) == 0
            assert lib.wsp_frontend_workspace_bytes(h, 4, 16000, ctypes.byref(b)) == 0
            assert lib.wsp_frontend_workspace_bytes(hh, 4, 16000, ctypes.byref(bh)) == 0
            rows = 4 * 49
            assert 0 < b.value - bh.value <= (rows * 12 + 63) // 64 * 64 * 4 + 256
        finally:
            lib.wsp_model_destroy(hh)
    finally:
        lib.wsp_model_destroy(h)


def test_wavlm_rejects_other_sizes():
    lib = _lib.load()
    h = ctypes.c_void_p()
    assert lib.wsp_model_create(b"WavLM_base", 1, 512, 0, 0, ctypes.byref(h)) != 0
    assert b"768" in lib.wsp_last_error()
    for arch in (b"WavLM_large", b"wavlm_base", b"WavLM"):
        assert lib.wsp_model_create(arch, 1, 768, 0, 0, ctypes.byref(h)) != 0
        assert b"unsupported arch" in lib.wsp_last_error()


def test_hubert_layout_unchanged():
    lib = _lib.load()
    h = ctypes.c_void_p()
    assert lib.wsp_model_create(b"HuBERT_base", 1, 768, 0, 0, ctypes.byref(h)) == 0
    try:
        got = _layout(lib, h)
    finally:
        lib.wsp_model_destroy(h)
    assert got == [(n, tuple(s)) for n, s in hubert_params()]
    assert not any("grep" in n or "relative_attention_bias" in n for n, _ in got)
