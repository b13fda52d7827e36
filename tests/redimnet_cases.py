"""The ReDimNetB2 reference fixtures (tests/golden/redimnet_*.npz, made by
tests/golden/make_redimnet_golden.py) and how a test rebuilds a fixture's weights and input from
its seeds.  Shared by the CPU and the GPU tests; no library or device is touched here."""
import glob
import os

import numpy as np

from wespeaker_hubert_amd import arch as A
from wespeaker_hubert_amd.synthetic import synth_feats, synth_state_dict

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
FIXTURES = sorted(glob.glob(os.path.join(GOLD, "redimnet_b*.npz")))
IDS = [os.path.basename(p)[:-4] for p in FIXTURES]
ARCH = "ReDimNetB2"
SEED = 87  # every fixture's weight seed
TAPS = ("stem",) + tuple(f"stage{i}" for i in range(6))


def synth_case(wseed, iseed, B, T, embed_dim=192, two_emb=False, scales=None):
    """(spec, parameter list, state dict, input) from seeds; `scales` multiplies each utterance."""
    spec = A.make_spec(ARCH, feat_dim=72, embed_dim=embed_dim, two_emb_layer=two_emb)
    plist = A.redimnet_params(spec)
    sd = synth_state_dict(wseed, plist)
    x = synth_feats(iseed, B, T, 72)
    if scales is not None:
        x = (x * np.asarray(scales, np.float32)[:, None, None]).astype(np.float32)
    return spec, plist, sd, x


def load_case(path):
    """(fixture, spec, parameter list, state dict, input features) of one fixture."""
    z = np.load(path, allow_pickle=False)
    assert str(z["arch"]) == ARCH and int(z["feat_dim"]) == 72
    spec, plist, sd, x = synth_case(int(z["weight_seed"]), int(z["input_seed"]), int(z["B"]), int(z["T"]),
                                    int(z["embed_dim"]), bool(int(z["two_emb"])), z["input_scales"])
    assert abs(float(x.astype(np.float64).sum()) - float(z["input_sum"])) < 1e-9
    assert np.array_equal(x.reshape(-1)[:16], z["input_head"])
    return z, spec, plist, sd, x
