"""Generate the x-vector / xi-vector golden fixtures from the REFERENCE implementation (survey container only).

    python tests/golden/make_xvec_golden.py

Imports `wespeaker/models/tdnn.py`, `xi_vector.py` and `ecapa_tdnn.py` read-only from
`/root/reference` (the package-init bypass of make_campplus_golden.py), loads seeded synthetic weights
(`synthetic.synth_state_dict`, keyed by parameter name, weight seed 83 for every case), runs the model
in eval mode on seeded features (times `input_scale`) and stores only seeds, input checksums and
outputs: `tests/golden/xvec_*.npz` / `xi_*.npz` with the keys of the other model fixtures plus the
float64 sum and abs-sum (`sum_<name>`, `abs_<name>`) of the pooling layer's output (and of frames 1,
3, 5 of the TDNN).  `embed` is the reference's outputs[-1] (embed_b for the TDNN).  No reference
source is copied.
"""
from __future__ import annotations

import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, REPO)

from wespeaker_hubert_amd.synthetic import synth_feats, synth_state_dict  # noqa: E402

REF = "/root/reference"
WEIGHT_SEED = 83

# (fixture, constructor, feat_dim, embed_dim, emb_bn, B, T, input scale); input seed 830 + i
CASES = [
    ("xvec_f80_e512_b2_t200", "XVEC", 80, 512, False, 2, 200, 1.0),             # the recipe shape
    ("xvec_f40_e256_b3_t16", "XVEC", 40, 256, False, 3, 16, 1.0),               # T' = 2, the smallest TSTP input
    ("xvec_f80_e512_b1_t37", "XVEC", 80, 512, False, 1, 37, 1.0),
    ("xi_xvec_f80_e512_b2_t15", "XI_VEC_XVEC", 80, 512, False, 2, 15, 1.0),     # T' = 1: the prior carries real weight
    ("xi_xvec_f80_e512_b2_t200", "XI_VEC_XVEC", 80, 512, False, 2, 200, 1.0),
    ("xi_ecapa512_f80_e192_b2_t200", "XI_VEC_ECAPA_TDNN_c512", 80, 192, False, 2, 200, 1.0),  # the recipe shape
    ("xi_ecapa512_f80_e192_bn_b1_t33", "XI_VEC_ECAPA_TDNN_c512", 80, 192, True, 1, 33, 1.0),
    ("xi_ecapa1024_f80_e256_b1_t150", "XI_VEC_ECAPA_TDNN_c1024", 80, 256, False, 1, 150, 1.0),
    ("xi_xvec_f80_e512_b2_t50_x8", "XI_VEC_XVEC", 80, 512, False, 2, 50, 8.0),  # large logits
    ("xi_ecapa512_f80_e192_b2_t50_x8", "XI_VEC_ECAPA_TDNN_c512", 80, 192, False, 2, 50, 8.0),
]


def main():
    pkg = types.ModuleType("wespeaker")
    pkg.__path__ = [os.path.join(REF, "wespeaker")]
    sys.modules["wespeaker"] = pkg
    from wespeaker.models import tdnn, xi_vector
    for i, (name, ctor, feat_dim, embed_dim, emb_bn, B, T, scale) in enumerate(CASES):
        wseed, iseed = WEIGHT_SEED, 830 + i
        torch.manual_seed(0)
        if ctor == "XVEC":
            model = tdnn.XVEC(feat_dim=feat_dim, embed_dim=embed_dim, pooling_func="TSTP").eval()
        elif ctor == "XI_VEC_XVEC":
            model = xi_vector.XI_VEC_XVEC(feat_dim=feat_dim, embed_dim=embed_dim).eval()
        else:
            model = getattr(xi_vector, ctor)(feat_dim=feat_dim, embed_dim=embed_dim, emb_bn=emb_bn).eval()
        shapes = [(k, tuple(v.shape)) for k, v in model.state_dict().items()]
        sd = synth_state_dict(wseed, shapes)
        model.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()}, strict=True)
        x = synth_feats(iseed, B, T, feat_dim) * np.float32(scale)
        rec = {}
        hooks = []

        def tap(mod, tag):
            def hook(_m, _i, o):
                rec["sum_" + tag] = np.float64(o.double().sum())
                rec["abs_" + tag] = np.float64(o.double().abs().sum())
            hooks.append(mod.register_forward_hook(hook))

        tap(model.pool, "pool")
        if hasattr(model, "frame_1"):
            for k in (1, 3, 5):
                tap(getattr(model, f"frame_{k}"), f"frame_{k}")
        with torch.no_grad():
            emb = model(torch.from_numpy(x.copy()))[-1]
        for h in hooks:
            h.remove()
        assert torch.isfinite(emb).all()
        rec.update(arch=np.array(ctor), weight_seed=np.int64(wseed), input_seed=np.int64(iseed), B=np.int64(B),
                   T=np.int64(T), feat_dim=np.int64(feat_dim), embed_dim=np.int64(embed_dim),
                   emb_bn=np.int64(emb_bn), input_scale=np.float64(scale),
                   input_sum=np.float64(x.astype(np.float64).sum()), input_head=x.reshape(-1)[:16].copy(),
                   param_names=np.array([k for k, _ in shapes]),
                   param_shapes=np.array([",".join(map(str, s)) for _, s in shapes]),
                   embed=emb.numpy().astype(np.float32))
        np.savez_compressed(os.path.join(HERE, name + ".npz"), **rec)
        print(name, len(shapes), tuple(emb.shape), float(emb.abs().max()), float(emb.pow(2).mean().sqrt()))


if __name__ == "__main__":
    main()
