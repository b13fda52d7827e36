"""Generate the Gemini DF-ResNet golden fixtures from the REFERENCE implementation (survey container only).

    python tests/golden/make_gemini_golden.py

Imports `wespeaker/models/gemini_dfresnet.py` read-only from `/root/reference` (the package-init
bypass of make_campplus_golden.py), loads seeded synthetic weights (`synthetic.synth_state_dict`,
keyed by parameter name, residual_tame=True, weight seed 71 for every case), runs the model in eval
mode on seeded features and stores only seeds, input checksums and outputs:
`tests/golden/gemini*.npz` with the keys of the other model fixtures plus the float64 sum and
abs-sum (`sum_<name>`, `abs_<name>`) of the stem, of the four downsample outputs and of the four
stages.  `embed` is the reference's outputs[-1] (embed_b with two_emb_layer).  No reference source
is copied.
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
WEIGHT_SEED = 71

# (fixture, constructor, feat_dim, embed_dim, two_emb_layer, B, T); input seed 720 + i
CASES = [
    ("gemini114_f80_e256_b2_t200", "Gemini_DF_ResNet114", 80, 256, False, 2, 200),   # the recipe shape
    ("gemini60_f80_e256_b1_t37", "Gemini_DF_ResNet60", 80, 256, False, 1, 37),       # odd T, 37 -> 19
    ("gemini60_f16_e64_b3_t3", "Gemini_DF_ResNet60", 16, 64, False, 3, 3),           # F' = 1, T' = 2: the smallest input
    ("gemini60_f32_e128_2emb_b2_t50", "Gemini_DF_ResNet60", 32, 128, True, 2, 50),
    ("gemini183_f80_e192_b1_t101", "Gemini_DF_ResNet183", 80, 192, False, 1, 101),
    ("gemini237_f80_e256_b1_t38", "Gemini_DF_ResNet237", 80, 256, False, 1, 38),     # 63 blocks in one stage
]


def main():
    pkg = types.ModuleType("wespeaker")
    pkg.__path__ = [os.path.join(REF, "wespeaker")]
    sys.modules["wespeaker"] = pkg
    from wespeaker.models import gemini_dfresnet
    for i, (name, ctor, feat_dim, embed_dim, two_emb, B, T) in enumerate(CASES):
        wseed, iseed = WEIGHT_SEED, 720 + i
        torch.manual_seed(0)
        model = getattr(gemini_dfresnet, ctor)(feat_dim=feat_dim, embed_dim=embed_dim, two_emb_layer=two_emb).eval()
        shapes = [(k, tuple(v.shape)) for k, v in model.state_dict().items()]
        sd = synth_state_dict(wseed, shapes, residual_tame=True)
        model.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()}, strict=True)
        x = synth_feats(iseed, B, T, feat_dim)
        rec = {}
        hooks = []

        def tap(mod, tag):
            def hook(_m, _i, o):
                rec["sum_" + tag] = np.float64(o.double().sum())
                rec["abs_" + tag] = np.float64(o.double().abs().sum())
            hooks.append(mod.register_forward_hook(hook))

        tap(model.downsample_layers[0], "stem")
        for li in (1, 2, 3, 4):
            tap(model.downsample_layers[li], f"down{li}")
            tap(model.stages[li - 1], f"stage{li}")
        with torch.no_grad():
            emb = model(torch.from_numpy(x.copy()))[-1]
        for h in hooks:
            h.remove()
        assert torch.isfinite(emb).all()
        rec.update(arch=np.array(ctor), weight_seed=np.int64(wseed), input_seed=np.int64(iseed), B=np.int64(B),
                   T=np.int64(T), feat_dim=np.int64(feat_dim), embed_dim=np.int64(embed_dim),
                   two_emb=np.int64(two_emb), residual_tame=np.int64(1),
                   input_sum=np.float64(x.astype(np.float64).sum()), input_head=x.reshape(-1)[:16].copy(),
                   param_names=np.array([k for k, _ in shapes]),
                   param_shapes=np.array([",".join(map(str, s)) for _, s in shapes]),
                   embed=emb.numpy().astype(np.float32))
        np.savez_compressed(os.path.join(HERE, name + ".npz"), **rec)
        print(name, tuple(emb.shape), float(emb.abs().max()), float(emb.pow(2).mean().sqrt()))


if __name__ == "__main__":
    main()
