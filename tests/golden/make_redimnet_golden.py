"""Generate the ReDimNetB2 golden fixtures from the REFERENCE implementation (survey container only).

    python tests/golden/make_redimnet_golden.py

Imports `wespeaker/models/redimnet.py` read-only from `/root/reference` (the package-init bypass of
make_campplus_golden.py), loads seeded synthetic weights (`synthetic.synth_state_dict`, keyed by
parameter name, weight seed 87 for every case), runs the model in eval mode on seeded features and
stores only seeds, input checksums and outputs: `tests/golden/redimnet_*.npz` with the keys of the
other model fixtures plus the float64 sum and abs-sum (`sum_<name>`, `abs_<name>`) of the stem and of
each stage, taken from the module in `.double()`.  `embed` is the reference's float32 outputs[-1]
(embed_b with two_emb_layer), `embed64` the same module's in float64.  No reference source is copied.

The weight seed was chosen on the reference's own error, before any device run: with seed 83 the T = 2
case puts a pooled variance at ASTP's 1e-7 clamp, where E[x^2] - mean^2 cancels and the reference's
own float32 embedding is 1.0e-5 off its float64 one; seeds 84..87 give 3.5e-6 .. 6.0e-6 there, and 87
keeps every case within 4.6e-6 (printed below), which is what the tests' bars are sized for.
"""
from __future__ import annotations

import copy
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
WEIGHT_SEED = 87
FEAT = 72

# (fixture, embed_dim, two_emb_layer, B, T, per-utterance input scales or None); input seed 830 + i
CASES = [
    ("redimnet_b2_t200", 192, False, 2, 200, None),          # the recipe shape
    ("redimnet_b3_t2", 192, False, 3, 2, None),              # the minimum T
    ("redimnet_b1_t30", 192, False, 1, 30, None),            # k59's +-29 taps land in range exactly once
    ("redimnet_b1_t37_e256_2emb", 256, True, 1, 37, None),   # odd T, two_emb_layer
    ("redimnet_b2_t301", 192, False, 2, 301, None),          # past 256 frames, odd T
    ("redimnet_b3_t64_mixed", 192, False, 3, 64, (0.0, 100.0, 0.01)),  # the stem LayerNorm's eps / range
]


def case_input(seed, B, T, scales):
    x = synth_feats(seed, B, T, FEAT)
    if scales is not None:
        x = (x * np.asarray(scales, np.float32)[:, None, None]).astype(np.float32)
    return x


def main():
    pkg = types.ModuleType("wespeaker")
    pkg.__path__ = [os.path.join(REF, "wespeaker")]
    sys.modules["wespeaker"] = pkg
    from wespeaker.models import redimnet
    for i, (name, embed_dim, two_emb, B, T, scales) in enumerate(CASES):
        wseed, iseed = WEIGHT_SEED, 830 + i
        torch.manual_seed(0)
        model = redimnet.ReDimNetB2(feat_dim=FEAT, embed_dim=embed_dim, two_emb_layer=two_emb).eval()
        shapes = [(k, tuple(v.shape)) for k, v in model.state_dict().items()]
        sd = synth_state_dict(wseed, shapes)
        model.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()}, strict=True)
        x = case_input(iseed, B, T, scales)
        with torch.no_grad():
            emb = model(torch.from_numpy(x.copy()))[-1]
        m64 = copy.deepcopy(model).double()
        rec = {}
        hooks = []

        def tap(mod, tag):
            def hook(_m, _i, o):
                rec["sum_" + tag] = np.float64(o.sum())
                rec["abs_" + tag] = np.float64(o.abs().sum())
            hooks.append(mod.register_forward_hook(hook))

        tap(m64.backbone.stem, "stem")
        for si in range(6):
            tap(getattr(m64.backbone, f"stage{si}"), f"stage{si}")
        with torch.no_grad():
            emb64 = m64(torch.from_numpy(x.copy()).double())[-1]
        for h in hooks:
            h.remove()
        assert torch.isfinite(emb).all() and torch.isfinite(emb64).all()
        rec.update(arch=np.array("ReDimNetB2"), weight_seed=np.int64(wseed), input_seed=np.int64(iseed), B=np.int64(B),
                   T=np.int64(T), feat_dim=np.int64(FEAT), embed_dim=np.int64(embed_dim), two_emb=np.int64(two_emb),
                   input_scales=np.asarray(scales if scales is not None else [1.0] * B, np.float32),
                   input_sum=np.float64(x.astype(np.float64).sum()), input_head=x.reshape(-1)[:16].copy(),
                   param_names=np.array([k for k, _ in shapes]),
                   param_shapes=np.array([",".join(map(str, s)) for _, s in shapes]),
                   embed=emb.numpy().astype(np.float32), embed64=emb64.numpy().astype(np.float64))
        np.savez_compressed(os.path.join(HERE, name + ".npz"), **rec)
        print(name, tuple(emb.shape), float(emb.abs().max()), float(emb.pow(2).mean().sqrt()),
              "f32 vs f64", float((emb.double() - emb64).abs().max()))


if __name__ == "__main__":
    main()
