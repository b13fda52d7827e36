"""The Res2Net reference fixtures (tests/golden/res2net_*.npz, made by
tests/golden/make_res2net_golden.py) and how a test rebuilds a fixture's weights and input from
its seeds.  Shared by the CPU and the GPU tests; no library or device is touched here."""
import glob
import os

import numpy as np

from wespeaker_hubert_amd import arch as A
from wespeaker_hubert_amd.synthetic import synth_feats, synth_state_dict

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
FIXTURES = sorted(glob.glob(os.path.join(GOLD, "res2net_*.npz")))
IDS = [os.path.basename(p)[:-4] for p in FIXTURES]


def synth_case(arch, wseed, iseed, B, T, feat_dim, embed_dim, two_emb=False, scale=1.0):
    """(spec, parameter list, state dict, input) from seeds: tamed synthetic weights, input x scale."""
    spec = A.make_spec(arch, feat_dim=feat_dim, embed_dim=embed_dim, two_emb_layer=two_emb)
    plist = A.res2net_params(spec)
    sd = synth_state_dict(wseed, plist, residual_tame=True)
    x = synth_feats(iseed, B, T, feat_dim) * np.float32(scale)
    return spec, plist, sd, x


def load_case(path):
    """(fixture, spec, parameter list, state dict, input features) of one fixture."""
    z = np.load(path, allow_pickle=False)
    assert int(z["residual_tame"]) == 1
    spec, plist, sd, x = synth_case(str(z["arch"]), int(z["weight_seed"]), int(z["input_seed"]), int(z["B"]),
                                    int(z["T"]), int(z["feat_dim"]), int(z["embed_dim"]), bool(int(z["two_emb"])),
                                    float(z["input_scale"]))
    return z, spec, plist, sd, x
