"""The CAM++ reference fixtures (tests/golden/campplus_*.npz, made by
tests/golden/make_campplus_golden.py) and how a test rebuilds a fixture's weights and input from
its seeds.  Shared by the CPU and the GPU tests; no library or device is touched here."""
import glob
import os

import numpy as np

from wespeaker_hubert_amd import arch as A
from wespeaker_hubert_amd.synthetic import synth_feats, synth_state_dict

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
FIXTURES = sorted(glob.glob(os.path.join(GOLD, "campplus_*.npz")))
IDS = [os.path.basename(p)[:-4] for p in FIXTURES]


def load_case(path):
    """(fixture, spec, parameter list, state dict, input features) of one fixture."""
    z = np.load(path, allow_pickle=False)
    spec = A.make_spec(str(z["arch"]), feat_dim=int(z["feat_dim"]), embed_dim=int(z["embed_dim"]))
    plist = A.campplus_params(spec)
    assert int(z["residual_tame"]) == 0
    sd = synth_state_dict(int(z["weight_seed"]), plist)
    x = synth_feats(int(z["input_seed"]), int(z["B"]), int(z["T"]), int(z["feat_dim"]))
    return z, spec, plist, sd, x
