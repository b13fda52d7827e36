"""Generate the CAM++ golden fixtures from the REFERENCE implementation (survey container only).

    python tests/golden/make_campplus_golden.py

Imports `wespeaker/models/campplus.py` read-only from `/root/reference` (the package-init
bypass of make_golden.py), loads seeded synthetic weights (`synthetic.synth_state_dict`, keyed
by parameter name, no residual taming), runs `CAMPPlus(...).eval()` on seeded features and stores
only seeds, input checksums and outputs: `tests/golden/campplus_*.npz` with the keys of the other
model fixtures plus, from forward hooks, the sum and abs-sum of the FCM output, of xvector.tdnn,
of each dense block and each transit (`sum_<name>`, `abs_<name>`, float64) and rows 0 and last of
`get_frame_level_feat` (`frame_first`, `frame_last`, [B][512]).  No reference source is copied.
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

# (fixture, feat_dim, embed_dim, weight seed, input seed, B, T)
CASES = [
    ("campplus_f80_e512_b2_t200", 80, 512, 41, 401, 2, 200),  # T' = 100: one full segment
    ("campplus_f80_e192_b1_t301", 80, 192, 42, 402, 1, 301),  # T' = 151
    ("campplus_f80_e512_b1_t403", 80, 512, 41, 403, 1, 403),  # T' = 202: a 2-frame last segment
    ("campplus_f40_e256_b2_t3", 40, 256, 43, 404, 2, 3),      # T' = 2
    ("campplus_f8_e64_b3_t201", 8, 64, 44, 405, 3, 201),      # T' = 101: a 1-frame last segment, F/8 = 1
]
TAPS = (("head", "head"), ("tdnn", "xvector.tdnn"), ("block1", "xvector.block1"), ("transit1", "xvector.transit1"),
        ("block2", "xvector.block2"), ("transit2", "xvector.transit2"), ("block3", "xvector.block3"),
        ("transit3", "xvector.transit3"))


def main():
    pkg = types.ModuleType("wespeaker")
    pkg.__path__ = [os.path.join(REF, "wespeaker")]
    sys.modules["wespeaker"] = pkg
    from wespeaker.models import campplus
    for name, feat_dim, embed_dim, wseed, iseed, B, T in CASES:
        torch.manual_seed(0)
        model = campplus.CAMPPlus(feat_dim=feat_dim, embed_dim=embed_dim).eval()
        shapes = [(k, tuple(v.shape)) for k, v in model.state_dict().items()]
        sd = synth_state_dict(wseed, shapes)
        model.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()}, strict=True)
        x = synth_feats(iseed, B, T, feat_dim)
        rec = {}
        hooks = []
        mods = dict(model.named_modules())
        for tag, mname in TAPS:
            def hook(_m, _i, o, tag=tag):
                # get_frame_level_feat below runs the modules again: keep the first (forward) pass
                rec.setdefault("sum_" + tag, np.float64(o.double().sum()))
                rec.setdefault("abs_" + tag, np.float64(o.double().abs().sum()))
            hooks.append(mods[mname].register_forward_hook(hook))
        with torch.no_grad():
            emb = model(torch.from_numpy(x))
            frames = model.get_frame_level_feat(torch.from_numpy(x))
        for h in hooks:
            h.remove()
        rec.update(arch=np.array("CAMPPlus"), weight_seed=np.int64(wseed), input_seed=np.int64(iseed), B=np.int64(B),
                   T=np.int64(T), feat_dim=np.int64(feat_dim), embed_dim=np.int64(embed_dim),
                   residual_tame=np.int64(0), input_sum=np.float64(x.astype(np.float64).sum()),
                   input_head=x.reshape(-1)[:16].copy(), param_names=np.array([k for k, _ in shapes]),
                   param_shapes=np.array([",".join(map(str, s)) for _, s in shapes]),
                   embed=emb.numpy().astype(np.float32),
                   frame_first=frames[:, 0].numpy().astype(np.float32),
                   frame_last=frames[:, -1].numpy().astype(np.float32))
        np.savez_compressed(os.path.join(HERE, name + ".npz"), **rec)
        print(name, tuple(emb.shape), float(emb.abs().max()), float(emb.abs().mean()))


if __name__ == "__main__":
    main()
