"""The x-vector / xi-vector reference fixtures (tests/golden/xvec_*.npz and xi_*.npz, made by
tests/golden/make_xvec_golden.py) and how a test rebuilds a fixture's weights and input from its
seeds.  Shared by the CPU and the GPU tests; no library or device is touched here."""
import glob
import os

import numpy as np

from wespeaker_hubert_amd import arch as A
from wespeaker_hubert_amd.synthetic import synth_feats, synth_state_dict

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
FIXTURES = sorted(glob.glob(os.path.join(GOLD, "xvec_f*.npz")) + glob.glob(os.path.join(GOLD, "xi_*_f*.npz")))
IDS = [os.path.basename(p)[:-4] for p in FIXTURES]
SEED = 83  # every fixture's weight seed


def synth_case(arch, wseed, iseed, B, T, feat_dim, embed_dim, emb_bn=False, scale=1.0, pooling_func=None):
    """(spec, parameter list, state dict, input) from seeds; `scale` multiplies the input."""
    kw = dict(feat_dim=feat_dim, embed_dim=embed_dim)
    if emb_bn:
        kw["emb_bn"] = True
    if pooling_func:
        kw["pooling_func"] = pooling_func
    spec = A.make_spec(arch, **kw)
    plist = A.param_list(spec)
    sd = synth_state_dict(wseed, plist)
    x = synth_feats(iseed, B, T, feat_dim) * np.float32(scale)
    return spec, plist, sd, x


def load_case(path):
    """(fixture, spec, parameter list, state dict, input features) of one fixture."""
    z = np.load(path, allow_pickle=False)
    spec, plist, sd, x = synth_case(str(z["arch"]), int(z["weight_seed"]), int(z["input_seed"]), int(z["B"]),
                                    int(z["T"]), int(z["feat_dim"]), int(z["embed_dim"]), bool(int(z["emb_bn"])),
                                    float(z["input_scale"]))
    return z, spec, plist, sd, x
