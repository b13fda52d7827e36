"""Op-level cases of the Res2Net kernels (tools/res2net_oprun): the fused block tail
(launch_res2_tail) and the 1x1 conv over a concatenated operand (launch_eres_pw with ksplit).
Shared by tests/test_res2net_op_ref_cpu.py and tests/test_gpu_res2net_op.py; no device is touched here.
Headers follow the op table in the head comment of tools/res2net_oprun.cpp."""
import numpy as np

import conv_gemm_ref as ref

MAGIC = 0x32505357
NH, OWN, NARRAYS = 16, 0, 1  # tools/res2net_oprun.cpp's Layout
OP_TAIL, OP_PW = 1, 2
NONE, RELU, CLAMP = 0, 1, 2

WIDTHS = (16, 32, 64, 128, 256)
# (B, F, T): the T' = 2 plane; two utterances of an odd plane; 105 positions (a tile tail in every wave:
# 16 and 32 positions per wave both leave one); 520 positions (more than one block of 64 or 128)
PLANES = ((1, 1, 2), (2, 3, 5), (3, 5, 7), (2, 10, 26))


def tail_case(seed, B, F, T, w, res, hot=False, pad=False):
    """y [M][ldy] holds post-clamp activations (half of them zero).  hot: y x 8 and biases around the
    ceiling, so that s and out fall on both sides of 20.  pad: strides wider than the rows, the output
    slice at a non-zero column."""
    rng = np.random.default_rng(seed)
    N, M = 4 * w, B * F * T
    ldy = 2 * w + (8 if pad else 0)
    ldo, ooff = (N + 12, 4) if pad else (N, 0)
    ldres = N + (4 if pad else 0)
    c = dict(op=OP_TAIL, hdr=[B, F, T, w, N, ldy, ldo, ooff, int(res), ldres if res else 0], B=B, F=F, T=T, w=w, N=N,
             M=M, ldy=ldy, ldo=ldo, ooff=ooff, ldres=ldres, hot=hot, has_res=res)
    c["y"] = ref.rand_a(rng, M, ldy, relu=True) * np.float32(8.0 if hot else 1.0)
    c["w1"] = ref.rand_w(rng, w, w, 3, 3)
    c["b1"] = rng.uniform(15.0, 25.0, w).astype(np.float32) if hot else ref.rand_w(rng, w, amp=0.3)
    c["w3"] = ref.rand_w(rng, N, 2 * w)
    c["b3"] = rng.uniform(15.0, 25.0, N).astype(np.float32) if hot else ref.rand_w(rng, N, amp=0.3)
    c["arrays"] = [c["y"], c["w1"], c["b1"], c["w3"], c["b3"]]
    if res:
        c["res"] = ref.rand_a(rng, M, ldres)
        c["arrays"].append(c["res"])
    return c


def pw_case(seed, B, Fi, Ti, cin, N, ksplit, stride=1, act=CLAMP, res=True, taps=1, null_a2=False, pad=False):
    """a [rows][lda] and a2 [rows][lda2] both hold cin columns, whatever ksplit says: a launch that is
    not refused reads a[:, :ksplit] and a2[:, :cin - ksplit] only."""
    rng = np.random.default_rng(seed)
    lda, lda2 = cin + (8 if pad else 0), cin + (4 if pad else 0)
    Fo, To = (Fi - 1) // stride + 1, (Ti - 1) // stride + 1
    M = B * Fo * To
    ldo, ooff = (N + 8, 4) if pad else (N, 0)
    c = dict(op=OP_PW, hdr=[taps, B, Fi, Ti, cin, N, stride, ksplit, lda, lda2, ldo, ooff, act, int(res), int(null_a2)],
             taps=taps, B=B, Fi=Fi, Ti=Ti, Fo=Fo, To=To, M=M, cin=cin, N=N, stride=stride, ksplit=ksplit, lda=lda,
             lda2=lda2, ldo=ldo, ooff=ooff, act=act, has_res=res)
    c["a"] = ref.rand_a(rng, B * Fi * Ti, lda, relu=True)
    c["a2"] = ref.rand_a(rng, B * Fi * Ti, lda2, relu=True)
    k = 3 if taps == 9 else 1
    c["w"] = ref.rand_w(rng, N, cin, k, k)
    c["bias"] = ref.rand_w(rng, N, amp=0.3)
    c["arrays"] = [c["a"], c["a2"], c["w"], c["bias"]]
    if res:
        c["res"] = ref.rand_a(rng, M, N)
        c["arrays"].append(c["res"])
    return c


TAIL_CASES = []
for _i, _w in enumerate(WIDTHS):
    for _j, (_B, _F, _T) in enumerate(PLANES):
        for _r in (False, True):
            TAIL_CASES.append(tail_case(100 * _i + 10 * _j + int(_r), _B, _F, _T, _w, _r, pad=(_j + int(_r)) % 2 == 1))
    # s and out on both sides of the ceiling
    TAIL_CASES.append(tail_case(100 * _i + 90, 2, 3, 5, _w, True, hot=True))

PW_CASES = []
for _i, (_cin, _ks) in enumerate(((32, 16), (64, 32), (512, 256))):  # 32 / 16: both sources inside one k-step
    for _st in (1, 2):
        PW_CASES.append(pw_case(500 + 10 * _i + _st, 2, 5, 7, _cin, 2 * _cin, _ks, stride=_st, pad=_st == 2))
PW_CASES.append(pw_case(540, 1, 3, 43, 64, 64, 24, res=False))  # a split inside a k-step that is no multiple of 16

# what launch_eres_pw / launch_eres_conv3x3 must refuse (status 1 and a message)
REFUSED = [
    (pw_case(600, 1, 2, 3, 32, 32, 12), "multiple of 8"),
    (pw_case(601, 1, 2, 3, 32, 32, 32), "multiple of 8 below cin"),
    (pw_case(602, 1, 2, 3, 32, 32, 16, null_a2=True), "second operand"),
    (pw_case(603, 1, 2, 3, 32, 32, 16, taps=9, res=False), "1x1 conv only"),
]

CASES = TAIL_CASES + PW_CASES + [c for c, _ in REFUSED]
