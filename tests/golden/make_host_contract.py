"""Records the host-only contract of the library's model handles into host_contract.json:
option defaults, aliases, accepted / refused values with their messages, and every
workspace query on a fixed grid.  None of the calls touches a GPU.

The fixture is recorded from the library of the commit BEFORE a host-code change and
checked against the library after it (tests/test_host_contract_cpu.py imports collect()
from here, so the two sides make the same calls):

    python tests/golden/make_host_contract.py --lib /path/to/old/libwsp_hip.so
"""
import argparse
import ctypes
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, "host_contract.json")

# name: (arch, feat_dim, embed_dim, emb_bn, two_emb)
HANDLES = {
    "ECAPA_TDNN_c512": ("ECAPA_TDNN_c512", 80, 192, 0, 0),
    "ECAPA_TDNN_GLOB_c1024+emb_bn": ("ECAPA_TDNN_GLOB_c1024", 80, 192, 1, 0),
    "ResNet18": ("ResNet18", 80, 256, 0, 0),
    "ResNet34+two_emb": ("ResNet34", 80, 256, 0, 1),
    "ResNet50": ("ResNet50", 80, 256, 0, 0),
    "ResNet293": ("ResNet293", 80, 256, 0, 0),
    "SimAM_ResNet34_ASP": ("SimAM_ResNet34_ASP", 80, 256, 0, 0),
    "SimAM_ResNet100_ASP+feat64": ("SimAM_ResNet100_ASP", 64, 256, 0, 0),
    "HuBERT_base": ("HuBERT_base", 1, 768, 0, 0),
    "WavLM_base": ("WavLM_base", 1, 768, 0, 0),
    "CAMPPlus": ("CAMPPlus", 80, 192, 0, 0),
}
# key: (a valid non-default-ish value, one value outside the accepted range)
OPTIONS = {
    "precision": (0, 2), "streams": (5, 0), "layer": (6, 13), "in_planes": (32, 48), "res2_fused": (0, 2),
    "cat_gate": (0, 2), "res_prefetch": (0, 2), "res_tail": (2, 3), "sc_fuse": (1, 4), "c1_stage_fuse": (0, 2),
    "astp_fused": (0, 4), "attn_pipe": (0, 2), "pos_conv": (0, 2), "ln_fold": (1, 2), "tail_batch": (0, 2),
    "res2_variant": (2, 1), "x3_variant": (3, 10), "conv3x3_img": (3, 4), "gate_fold": (0, 2), "cam_fused": (0, 2),
}
EXTRA_REFUSED = (("res2_variant", 5), ("x3_variant", -1), ("streams", 9), ("layer", -2), ("in_planes", 33))
X3_ALIASES = (0, 1, 2, 6, 8, 9)
ASTP_ALIASES = (2, 3)
GRID = ((1, 2), (1, 17), (3, 200), (7, 498), (256, 498), (640, 498))  # the last crosses the chunk rule
RAGGED_LENS = (16000, 399, 48000)


def collect(lib):
    """{handle name: recorded values} from `lib` (a ctypes.CDLL with _lib.SIGNATURES applied)."""
    v, nbytes = ctypes.c_int(), ctypes.c_size_t()

    def create(spec):
        h = ctypes.c_void_p()
        arch, feat, emb, emb_bn, two_emb = spec
        assert lib.wsp_model_create(arch.encode(), feat, emb, emb_bn, two_emb, ctypes.byref(h)) == 0, arch
        return h

    def get(h, key):
        rc = lib.wsp_model_get_option(h, key.encode(), ctypes.byref(v))
        return v.value if rc == 0 else {"rc": rc, "error": lib.wsp_last_error().decode()}

    def put(h, key, value):
        rc = lib.wsp_model_set_option(h, key.encode(), value)
        return {"rc": rc, "error": lib.wsp_last_error().decode() if rc else "", "readback": get(h, key)}

    def query(fn, h, *args):
        rc = fn(h, *args, ctypes.byref(nbytes))
        return nbytes.value if rc == 0 else {"rc": rc, "error": lib.wsp_last_error().decode()}

    def grid(h):
        lens = (ctypes.c_int * len(RAGGED_LENS))(*RAGGED_LENS)
        return {
            "model": [query(lib.wsp_model_workspace_bytes, h, b, t) for b, t in GRID],
            "model_segments_3_100": query(lib.wsp_model_workspace_bytes_segments, h, 3, 100),
            "frontend": [query(lib.wsp_frontend_workspace_bytes, h, b, 160 * t) for b, t in GRID],
            "frontend_segments": query(lib.wsp_frontend_workspace_bytes_segments, h, len(RAGGED_LENS), lens),
        }

    out = {}
    for name, spec in HANDLES.items():
        rec = {}
        h = create(spec)
        rec["num_params"] = lib.wsp_model_num_params(h)
        rec["defaults"] = {k: get(h, k) for k in OPTIONS}
        rec["workspace"] = {"default": grid(h)}
        for ns in (1, 3):
            assert lib.wsp_model_set_option(h, b"streams", ns) == 0
            rec["workspace"]["streams%d" % ns] = grid(h)
        lib.wsp_model_destroy(h)

        h = create(spec)
        rec["x3_variant_alias"] = {str(a): put(h, "x3_variant", a) for a in X3_ALIASES}
        rec["astp_fused_alias"] = {str(a): put(h, "astp_fused", a) for a in ASTP_ALIASES}
        rec["noop"] = {k: lib.wsp_model_set_option(h, k.encode(), 1) for k in ("attn_lds", "conv1x1_rows")}
        rec["noop_get"] = get(h, "attn_lds")
        rec["unknown_set"] = put(h, "no_such_option", 1)
        lib.wsp_model_destroy(h)

        h = create(spec)
        rec["refused"] = {"%s=%d" % (k, bad): put(h, k, bad) for k, (_, bad) in OPTIONS.items()}
        rec["refused"].update({"%s=%d" % (k, bad): put(h, k, bad) for k, bad in EXTRA_REFUSED})
        rec["after_refused"] = {k: get(h, k) for k in OPTIONS}
        lib.wsp_model_destroy(h)

        h = create(spec)
        rec["accepted"] = {"%s=%d" % (k, ok): put(h, k, ok) for k, (ok, _) in OPTIONS.items()}
        rec["num_params_after_accepted"] = lib.wsp_model_num_params(h)
        lib.wsp_model_destroy(h)
        out[name] = rec
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lib", required=True, help="library of the commit before the change under test")
    ap.add_argument("--out", default=OUT)
    a = ap.parse_args()
    sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
    from wespeaker_hubert_amd import _lib
    _lib.LIB_PATH = os.path.abspath(a.lib)
    with open(a.out, "w") as f:
        json.dump(collect(_lib.load()), f, indent=1, sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    main()
