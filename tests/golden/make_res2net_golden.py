"""Generate the Res2Net golden fixtures from the REFERENCE implementation (survey container only).

    python tests/golden/make_res2net_golden.py

Imports `wespeaker/models/res2net.py` read-only from `/root/reference` (the package-init bypass
of make_eres2net_golden.py), loads seeded synthetic weights (`synthetic.synth_state_dict`, keyed by
parameter name, residual_tame=True), runs the model in eval mode on seeded features (times
`input_scale`: the scaled cases drive activations into the Hardtanh ceiling) and stores only seeds,
input checksums and outputs: `tests/golden/res2net_*.npz` with the keys of the other model
fixtures plus the float64 sum and abs-sum (`sum_<name>`, `abs_<name>`) of the stem and of layer1..4
and, per stage, the number of elements equal to 20.0 at the stage output (`at20`).  A scaled case
must reach the ceiling in at least two stages, or the generator fails.  No reference source is copied.
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

# (fixture, constructor, feat_dim, embed_dim, two_emb_layer, B, T, input scale); weight seed 171 + i,
# input seed 1700 + i
CASES = [
    ("res2net_base_f80_e256_b2_t200", "Res2Net34_Base", 80, 256, False, 2, 200, 1.0),  # the recipe shape
    ("res2net_base_f80_e192_b1_t37", "Res2Net34_Base", 80, 192, False, 1, 37, 1.0),    # T odd at every level
    ("res2net_base_f8_e64_b3_t9", "Res2Net34_Base", 8, 64, False, 3, 9, 1.0),          # F' = 1, T' = 2
    ("res2net_base_f40_e256_2emb_b2_t50", "Res2Net34_Base", 40, 256, True, 2, 50, 1.0),
    ("res2net_large_f80_e256_b1_t101", "Res2Net34_Large", 80, 256, False, 1, 101, 1.0),
    ("res2net_base_f80_e256_b2_t200_x8", "Res2Net34_Base", 80, 256, False, 2, 200, 8.0),
    ("res2net_large_f80_e192_b1_t37_x8", "Res2Net34_Large", 80, 192, False, 1, 37, 8.0),
]


def run_case(res2net, ctor, feat_dim, embed_dim, two_emb, B, T, scale, wseed, iseed):
    torch.manual_seed(0)
    model = getattr(res2net, ctor)(feat_dim=feat_dim, embed_dim=embed_dim, two_emb_layer=two_emb).eval()
    shapes = [(k, tuple(v.shape)) for k, v in model.state_dict().items()]
    sd = synth_state_dict(wseed, shapes, residual_tame=True)
    model.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()}, strict=True)
    x = synth_feats(iseed, B, T, feat_dim) * np.float32(scale)
    rec, at20, hooks = {}, {}, []

    def tap(mod, tag):
        def hook(_m, _i, o):
            rec["sum_" + tag] = np.float64(o.double().sum())
            rec["abs_" + tag] = np.float64(o.double().abs().sum())
            at20[tag] = int((o == 20.0).sum())
        hooks.append(mod.register_forward_hook(hook))

    # the stem's ReLU is functional: record bn1's output through it
    hooks.append(model.bn1.register_forward_hook(lambda _m, _i, o: rec.update(
        sum_stem=np.float64(o.double().clamp_min(0).sum()), abs_stem=np.float64(o.double().clamp_min(0).sum()))))
    for li in (1, 2, 3, 4):
        tap(getattr(model, f"layer{li}"), f"layer{li}")
    with torch.no_grad():
        emb = model(torch.from_numpy(x.copy()))
    for h in hooks:
        h.remove()
    assert isinstance(emb, torch.Tensor) and torch.isfinite(emb).all()
    rec["at20"] = np.array([at20[f"layer{li}"] for li in (1, 2, 3, 4)], dtype=np.int64)
    return shapes, x, emb, rec


def main():
    pkg = types.ModuleType("wespeaker")
    pkg.__path__ = [os.path.join(REF, "wespeaker")]
    sys.modules["wespeaker"] = pkg
    from wespeaker.models import res2net
    for i, (name, ctor, feat_dim, embed_dim, two_emb, B, T, scale) in enumerate(CASES):
        wseed, iseed = 171 + i, 1700 + i
        while True:
            shapes, x, emb, rec = run_case(res2net, ctor, feat_dim, embed_dim, two_emb, B, T, scale, wseed, iseed)
            # a scaled case tests the clamp's ceiling only if the reference reaches it: raise the scale until
            # at least two stage outputs hold elements equal to 20.0
            if scale == 1.0 or int((rec["at20"] > 0).sum()) >= 2:
                break
            scale *= 2.0
            assert scale <= 1024.0, name
        rec.update(arch=np.array(ctor), weight_seed=np.int64(wseed), input_seed=np.int64(iseed), B=np.int64(B),
                   T=np.int64(T), feat_dim=np.int64(feat_dim), embed_dim=np.int64(embed_dim),
                   two_emb=np.int64(two_emb), input_scale=np.float64(scale), residual_tame=np.int64(1),
                   input_sum=np.float64(x.astype(np.float64).sum()), input_head=x.reshape(-1)[:16].copy(),
                   param_names=np.array([k for k, _ in shapes]),
                   param_shapes=np.array([",".join(map(str, s)) for _, s in shapes]),
                   embed=emb.numpy().astype(np.float32))
        np.savez_compressed(os.path.join(HERE, name + ".npz"), **rec)
        print(name, tuple(emb.shape), "scale", scale, "at20", rec["at20"].tolist(), float(emb.abs().max()),
              float(emb.pow(2).mean().sqrt()))


if __name__ == "__main__":
    main()
