"""Op-level cases of the RepVGG / RepSPK kernels (tools/repvgg_oprun): the 17-tap RepSPK block conv
(launch_rsbb_conv) and the stem (launch_repvgg_stem).  Shared by tests/test_repvgg_op_ref_cpu.py and
tests/test_gpu_repvgg_op.py; no device is touched here.  Headers follow the op table in the head comment
of tools/repvgg_oprun.cpp."""
import numpy as np

import conv_gemm_ref as ref

MAGIC = 0x56505357
NH, OWN, NARRAYS = 12, 0, 1  # tools/repvgg_oprun.cpp's Layout
OP_BLOCK, OP_STEM = 1, 2

# (cin, N, stride, channels of the model before padding): the four TINY stage shapes, and the padded widths
# 48 -> 48 (as 64 -> 64) and 48 -> 96 (as 64 -> 128), whose pad channels carry zero inputs, weights and bias
WIDTHS = ((32, 32, 1, None), (32, 64, 2, None), (64, 128, 2, None), (128, 256, 2, None), (64, 64, 1, (48, 48)),
          (64, 128, 2, (48, 96)))
# (B, F, T): the F' = 1, T' = 2 plane; a plane in which every output has taps outside it; a plane odd on both
# axes under stride 2; 500 positions (more than one 128-row block, with a tail)
PLANES = ((3, 1, 2), (2, 3, 5), (1, 5, 37), (2, 10, 25))


def fold5(w3, wd):
    """[n][c][3][3] x 2 -> the 5x5 kernel: the 3x3 at the inner taps plus the dilated 3x3 at the even taps."""
    w5 = np.zeros(w3.shape[:2] + (5, 5), np.float32)
    w5[:, :, 1:4, 1:4] += w3
    w5[:, :, ::2, ::2] += wd
    return w5


def block_case(seed, B, Fi, Ti, cin, N, stride, real=None, pad=False, ooff=None):
    """x [rows][ldx] post-ReLU activations; w3 / wd the two branches, w their 5x5 sum (dead taps zero)."""
    rng = np.random.default_rng(seed)
    ldx = cin + (8 if pad else 0)
    ldo, off = (N + 12, 4) if pad else (N, 0)
    if ooff is not None:
        ldo, off = N + 12, ooff
    Fo, To = (Fi - 1) // stride + 1, (Ti - 1) // stride + 1
    c = dict(op=OP_BLOCK, hdr=[B, Fi, Ti, cin, N, stride, ldx, ldo, off], B=B, Fi=Fi, Ti=Ti, Fo=Fo, To=To,
             M=B * Fo * To, cin=cin, N=N, stride=stride, ldx=ldx, ldo=ldo, ooff=off, real=real)
    c["x"] = ref.rand_a(rng, B * Fi * Ti, ldx, relu=True)
    c["w3"], c["wd"] = ref.rand_w(rng, N, cin, 3, 3), ref.rand_w(rng, N, cin, 3, 3)
    c["bias"] = ref.rand_w(rng, N, amp=0.3)
    if real:  # the channel padding of the model: zero inputs, zero weights, zero bias
        ci, co = real
        c["x"][:, ci:cin] = 0.0
        for k in ("w3", "wd"):
            c[k][co:] = 0.0
            c[k][:, ci:] = 0.0
        c["bias"][co:] = 0.0
    c["w"] = fold5(c["w3"], c["wd"])
    c["arrays"] = [c["x"], c["w"], c["bias"]]
    return c


def stem_case(seed, B, T, F, C0, taps, Cpad=None, pad=False):
    rng = np.random.default_rng(seed)
    Cpad = Cpad or C0
    ldo, off = (Cpad + 8, 4) if pad else (Cpad, 0)
    c = dict(op=OP_STEM, hdr=[B, T, F, C0, Cpad, taps, ldo, off], B=B, T=T, F=F, M=B * F * T, C0=C0, Cpad=Cpad, N=Cpad,
             taps=taps, ldo=ldo, ooff=off)
    c["feats"] = rng.standard_normal((B, T, F)).astype(np.float32)
    if taps == 9:
        c["w"] = ref.rand_w(rng, C0, 1, 3, 3, amp=0.3)
    elif taps == 17:
        c["w"] = fold5(ref.rand_w(rng, C0, 1, 3, 3, amp=0.3), ref.rand_w(rng, C0, 1, 3, 3, amp=0.3))
    else:
        c["w"] = ref.rand_w(rng, C0, 1, 5, 5, amp=0.3)
    c["bias"] = ref.rand_w(rng, C0, amp=0.3)
    c["arrays"] = [c["feats"], c["w"], c["bias"]]
    return c


BLOCK_CASES = []
for _i, (_cin, _N, _s, _real) in enumerate(WIDTHS):
    for _j, (_B, _F, _T) in enumerate(PLANES):
        BLOCK_CASES.append(block_case(100 * _i + _j, _B, _F, _T, _cin, _N, _s, _real, pad=(_i + _j) % 2 == 1))

STEM_CASES = []
for _i, _C0 in enumerate((32, 48, 64)):
    for _j, _taps in enumerate((9, 17)):
        for _k, _F in enumerate((8, 80)):
            # (B, T) = (3, 9) at feat_dim 8, (2, 13) at feat_dim 80: two blocks of 256 positions and a tail
            STEM_CASES.append(stem_case(700 + 10 * _i + 2 * _j + _k, 3 if _F == 8 else 2, 9 if _F == 8 else 13, _F, _C0,
                                        _taps, Cpad=64 if _C0 == 48 else None, pad=(_i + _j + _k) % 2 == 1))
STEM_CASES.append(stem_case(790, 2, 9, 8, 32, 25))  # the whole 5x5 (a checkpoint with non-zero dead taps)

# what the launchers must refuse (status 1 and a message)
REFUSED = [
    (block_case(900, 1, 3, 5, 32, 32, 3), "stride must be 1 or 2"),
    (block_case(901, 1, 3, 5, 48, 64, 1), "cin must be a multiple of 32"),
    (block_case(902, 1, 3, 5, 32, 32, 1, ooff=2), "16-byte aligned"),
    (stem_case(903, 1, 9, 8, 40, 9), "C0 must be 32, 48 or 64"),
]

CASES = BLOCK_CASES + STEM_CASES + [c for c, _ in REFUSED]
