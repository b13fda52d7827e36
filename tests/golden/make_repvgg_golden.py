"""Generate the RepVGG golden fixtures from the REFERENCE implementation (survey container only).

    python tests/golden/make_repvgg_golden.py

Imports `wespeaker/models/repvgg.py` read-only from `/root/reference` (the package-init bypass of
make_res2net_golden.py), loads seeded synthetic weights (`synthetic.synth_state_dict`, keyed by parameter
name, with the family's rule tests/repvgg_cases.py `tame`: branch BatchNorm scales x 0.65), runs the
training-form model and the model the reference's own `repvgg_model_convert` makes of it, both in eval
mode and float32, on seeded features and stores only seeds, input checksums and outputs:
`tests/golden/repvgg_*.npz` with the keys of the other model fixtures plus
  embed / embed_deploy          the two embeddings
  param_names_deploy / _shapes  the converted model's state_dict layout
  wsum_<b>_w / wabs_<b>_w / wsum_<b>_b / wabs_<b>_b   float64 sum and abs-sum of the converted
                                rbr_reparam.weight / .bias of b = stage0, stage1.0, stage3.0, last
  sum_<stage> / abs_<stage> / rms_<stage>   of the output of stage0 .. stage4 (training form)
Every stage rms must lie in [0.1, 10], or the generator fails: a later seed change cannot drift back into
the blown-up regime unnoticed.  No reference source is copied.
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
sys.path.insert(0, os.path.dirname(HERE))

from repvgg_cases import BN_SCALE, CHECKED_BLOCKS, tame  # noqa: E402
from wespeaker_hubert_amd.synthetic import synth_feats, synth_state_dict  # noqa: E402

REF = "/root/reference"

# (fixture, constructor, feat_dim, embed_dim, B, T); weight seed 191 + i, input seed 2100 + i
CASES = [
    ("repvgg_tiny_a0_f80_e256_b2_t200", "REPVGG_TINY_A0", 80, 256, 2, 200),       # the recipe shape
    ("repvgg_tiny_a0_f80_e192_b1_t37", "REPVGG_TINY_A0", 80, 192, 1, 37),         # T odd at every level
    ("repvgg_tiny_a0_f8_e64_b3_t9", "REPVGG_TINY_A0", 8, 64, 3, 9),               # F' = 1, T' = 2
    ("repvgg_tiny_rsbb_a0_f80_e256_b2_t200", "REPVGG_TINY_RSBB_A0", 80, 256, 2, 200),
    ("repvgg_tiny_rsbb_a0_f8_e64_b3_t9", "REPVGG_TINY_RSBB_A0", 8, 64, 3, 9),
    ("repvgg_a0_f80_e256_b1_t101", "REPVGG_A0", 80, 256, 1, 101),                 # widths 48 / 96 / 1280
    ("repvgg_rsbb_a2_f40_e256_b2_t50", "REPVGG_RSBB_A2", 40, 256, 2, 50),         # width 1408, 96-wide RepSPK
    ("repvgg_rsbb_b0_f80_e192_b1_t37", "REPVGG_RSBB_B0", 80, 192, 1, 37),
]


def sums(t):
    t = t.double()
    return np.float64(t.sum()), np.float64(t.abs().sum())


def run_case(repvgg, ctor, feat_dim, embed_dim, B, T, wseed, iseed):
    torch.manual_seed(0)
    model = getattr(repvgg, ctor)(feat_dim=feat_dim, embed_dim=embed_dim).eval()
    shapes = [(k, tuple(v.shape)) for k, v in model.state_dict().items()]
    sd = tame(synth_state_dict(wseed, shapes))
    model.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()}, strict=True)
    x = synth_feats(iseed, B, T, feat_dim)
    rec, hooks = {}, []
    for li in range(5):
        def hook(_m, _i, o, tag=f"stage{li}"):
            rec["sum_" + tag], rec["abs_" + tag] = sums(o)
            rec["rms_" + tag] = np.float64(o.double().pow(2).mean().sqrt())
        hooks.append(getattr(model, f"stage{li}").register_forward_hook(hook))
    with torch.no_grad():
        emb = model(torch.from_numpy(x.copy()))
    for h in hooks:
        h.remove()
    dep = repvgg.repvgg_model_convert(model).eval()
    with torch.no_grad():
        emb_d = dep(torch.from_numpy(x.copy()))
    dsd = dep.state_dict()
    dshapes = [(k, tuple(v.shape)) for k, v in dsd.items()]
    last = [k for k, _ in dshapes if k.endswith("rbr_reparam.weight")][-1][:-len(".rbr_reparam.weight")]
    for tag in CHECKED_BLOCKS:
        p = last if tag == "last" else tag
        rec[f"wsum_{tag}_w"], rec[f"wabs_{tag}_w"] = sums(dsd[p + ".rbr_reparam.weight"])
        rec[f"wsum_{tag}_b"], rec[f"wabs_{tag}_b"] = sums(dsd[p + ".rbr_reparam.bias"])
    for t in (emb, emb_d):
        assert isinstance(t, torch.Tensor) and torch.isfinite(t).all()
    for li in range(5):
        assert 0.1 <= float(rec[f"rms_stage{li}"]) <= 10.0, (ctor, li, float(rec[f"rms_stage{li}"]))
    return shapes, dshapes, x, emb, emb_d, rec


def main():
    pkg = types.ModuleType("wespeaker")
    pkg.__path__ = [os.path.join(REF, "wespeaker")]
    sys.modules["wespeaker"] = pkg
    from wespeaker.models import repvgg
    for i, (name, ctor, feat_dim, embed_dim, B, T) in enumerate(CASES):
        wseed, iseed = 191 + i, 2100 + i
        shapes, dshapes, x, emb, emb_d, rec = run_case(repvgg, ctor, feat_dim, embed_dim, B, T, wseed, iseed)
        rec.update(arch=np.array(ctor), weight_seed=np.int64(wseed), input_seed=np.int64(iseed), B=np.int64(B),
                   T=np.int64(T), feat_dim=np.int64(feat_dim), embed_dim=np.int64(embed_dim),
                   bn_scale=np.float64(BN_SCALE),
                   input_sum=np.float64(x.astype(np.float64).sum()), input_head=x.reshape(-1)[:16].copy(),
                   param_names=np.array([k for k, _ in shapes]),
                   param_shapes=np.array([",".join(map(str, s)) for _, s in shapes]),
                   param_names_deploy=np.array([k for k, _ in dshapes]),
                   param_shapes_deploy=np.array([",".join(map(str, s)) for _, s in dshapes]),
                   embed=emb.numpy().astype(np.float32), embed_deploy=emb_d.numpy().astype(np.float32))
        np.savez_compressed(os.path.join(HERE, name + ".npz"), **rec)
        print(name, tuple(emb.shape), "rms", [round(float(rec[f"rms_stage{li}"]), 3) for li in range(5)],
              "emb rms", float(emb.pow(2).mean().sqrt()), "train-deploy", float((emb - emb_d).abs().max()))


if __name__ == "__main__":
    main()
