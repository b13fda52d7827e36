"""The RepVGG reference fixtures (tests/golden/repvgg_*.npz, made by tests/golden/make_repvgg_golden.py)
and how a test rebuilds a fixture's weights and input from its seeds.  Shared by the generator, the CPU
and the GPU tests; no library or device is touched here.

Plain `synth_state_dict` weights do not suit this family: a block sums up to three BatchNorm-ed branches,
so the activations grow from block to block (stage-3 rms 2.3e5 in REPVGG_TINY_A0, where float32 itself is
off by 0.6).  The test-side rule `tame` multiplies every `*.bn.weight` and `*.rbr_identity.weight` by 0.65,
which keeps every stage's rms within 0.2 .. 2.1 and the embeddings at O(1) for the fixtures here (the generator
refuses anything outside 0.1 .. 10)."""
import glob
import os

import numpy as np

from wespeaker_hubert_amd import arch as A
from wespeaker_hubert_amd.synthetic import synth_feats, synth_state_dict

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
FIXTURES = sorted(glob.glob(os.path.join(GOLD, "repvgg_*.npz")))
IDS = [os.path.basename(p)[:-4] for p in FIXTURES]
BN_SCALE = np.float32(0.65)
# the converted tensors whose checksums a fixture stores
CHECKED_BLOCKS = ("stage0", "stage1.0", "stage3.0", "last")


def tame(sd):
    """The family's synthetic-weight rule, in place: every branch BatchNorm's scale times 0.65."""
    for k, v in sd.items():
        if k.endswith(".bn.weight") or k.endswith(".rbr_identity.weight"):
            sd[k] = (v * BN_SCALE).astype(np.float32)
    return sd


def synth_case(arch, wseed, iseed, B, T, feat_dim, embed_dim):
    """(training-form spec, parameter list, training-form state dict, input) from seeds."""
    spec = A.make_spec(arch, feat_dim=feat_dim, embed_dim=embed_dim)
    plist = A.repvgg_params(spec)
    sd = tame(synth_state_dict(wseed, plist))
    return spec, plist, sd, synth_feats(iseed, B, T, feat_dim)


def load_case(path):
    """(fixture, spec, parameter list, state dict, input features) of one fixture."""
    z = np.load(path, allow_pickle=False)
    assert float(z["bn_scale"]) == float(BN_SCALE)
    return (z,) + synth_case(str(z["arch"]), int(z["weight_seed"]), int(z["input_seed"]), int(z["B"]), int(z["T"]),
                             int(z["feat_dim"]), int(z["embed_dim"]))


def last_block(spec):
    return [p for p, *_ in A.repvgg_blocks(spec)][-1]
