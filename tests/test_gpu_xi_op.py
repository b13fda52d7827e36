"""Op-level conformance of XI pooling and the valid-conv offset tables against float64 (tools/xi_run).

The runner launches the shipped launch_xi_pool / launch_valid_conv_offsets of libwsp_hip.so and holds
no arithmetic of its own; every case runs in ONE runner process whose results the tests share.

XI cases: C in {64, 1500, 1536} with every leading dimension > C, T in {1, 2, 63, 64, 65, 257}, B = 3
uniform and ragged (lengths T, 1, (T + 1) // 2), logits ~ N(0, 1) and x 20 (both softplus branches,
exp(z) down to f32 subnormals), prior_logprec uniform in [-8, 8] with the two ends present.  Guard
rows and the columns past C must come back bit-untouched.

Allowance per output, first order, from the arithmetic xi_pool.hip performs.  Reference (f64):
phi = (sum_t w_t x_t + w_0 m) / W, w_t = softplus(z_t)^2 (z > 20: z), w_0 = exp(lp), W = sum_t w_t + w_0.
The kernel forms s~ = log1pf(expf(z)) in f32, everything after it in f64:
  * expf within 3 ulp and log1pf within 2 ulp (the OpenCL full-profile bounds the device library
    meets), and d log1p(e) / log1p(e) <= d e / e, so |s~ - s| <= ds = max(5 * 2^-23 s, 2^-149) (the
    second term: exp(z) itself subnormal); z > 20 is exact;
  * w~ = s~ s~ is exact in f64 (two 24-bit factors): |w~ - w| <= dw = 2 s ds + ds^2;
  * phi moves by sum_t (w~_t - w_t)(x_t - phi) / W to first order:  sum_t dw_t |x_t - phi| / W;
  * the f64 sums, exp(lp) and the division: (T + 3) 2^-52 sum_i w_i |v_i| / W;
  * the result is rounded to f32 once: 2^-24 |phi|.
Measured on an MI355X: max |err| / allowance = 0.988 over the 72 cases (max |err| 1.7e-7; where the
logits are x 20 a few frames carry all the weight and the allowance is little more than the final
f32 rounding of phi, which the kernel's result then nearly fills).  The offset tables are compared
exactly.
"""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import op_runner  # noqa: E402
from op_runner import FILL  # noqa: E402

MAGIC = 0x58505357
XI, OFFS = 1, 2

pytestmark = pytest.mark.gpu


def _xi_case(idx, C, T, ragged, zscale):
    rng = np.random.default_rng([97, idx])
    B = 3
    lens = [T, 1, (T + 1) // 2] if ragged else [T] * B
    seg = np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
    rows = int(seg[-1])
    ldz, ldx, ldo = C + 4, C + 8, C + 12
    z = (zscale * rng.standard_normal((rows, ldz))).astype(np.float32)
    x = rng.standard_normal((rows, ldx)).astype(np.float32)
    pm = rng.standard_normal(C).astype(np.float32)
    lp = rng.uniform(-8.0, 8.0, C).astype(np.float32)
    lp[0], lp[1] = 8.0, -8.0
    return dict(op=XI, hdr=[B, T, C, ldz, ldx, ldo, int(ragged), 0], B=B, T=T, C=C, ldo=ldo, seg=seg, ragged=ragged,
                z=z, x=x, pm=pm, lp=lp, zscale=zscale,
                arrays=[z, x, pm, lp, seg if ragged else np.zeros(0, np.int32)])


def _off_case(B, shrinks, seed):
    rng = np.random.default_rng([98, seed])
    off = np.concatenate([[0], np.cumsum(rng.integers(15, 600, B))]).astype(np.int32)
    hdr = [B, len(shrinks)] + list(shrinks) + [0] * (4 - len(shrinks)) + [0, 0]
    return dict(op=OFFS, hdr=hdr, B=B, shrinks=shrinks, off=off, arrays=[off])


CASES = []
for _C in (64, 1500, 1536):
    for _T in (1, 2, 63, 64, 65, 257):
        for _ragged in (False, True):
            for _zs in (1.0, 20.0):
                CASES.append(_xi_case(len(CASES), _C, _T, _ragged, _zs))
CASES += [_off_case(3, (4, 8, 14), 0), _off_case(1, (14,), 1), _off_case(700, (4, 8, 14, 0), 2)]


def _id(c):
    if c["op"] == OFFS:
        return f"offsets-b{c['B']}-n{len(c['shrinks'])}"
    return f"xi-c{c['C']}-t{c['T']}-{'ragged' if c['ragged'] else 'uniform'}-z{int(c['zscale'])}"


IDS = [_id(c) for c in CASES]


@pytest.fixture(scope="module")
def results(tmp_path_factory):
    """One runner process for all cases: (status, message, result words as uint32)."""
    out = op_runner.run("xi_run", MAGIC, [(c["op"], c["hdr"], c["arrays"]) for c in CASES],
                        tmp_path_factory.mktemp("xi_op"))
    return [(r["status"], r["message"], r["arrays"][0].view(np.uint32) if r["status"] == 0 else None) for r in out]


def xi_reference(c):
    """(phi in f64 [B][C], allowance [B][C]) — see the module docstring."""
    B, C, seg = c["B"], c["C"], c["seg"]
    phi, allow = np.zeros((B, C)), np.zeros((B, C))
    w0 = np.exp(c["lp"].astype(np.float64))
    m = c["pm"].astype(np.float64)
    for b in range(B):
        z = c["z"][seg[b]:seg[b + 1], :C].astype(np.float64)
        x = c["x"][seg[b]:seg[b + 1], :C].astype(np.float64)
        T = z.shape[0]
        s = np.where(z > 20.0, z, np.log1p(np.exp(np.minimum(z, 20.0))))
        w = s * s
        W = w.sum(0) + w0
        p = ((w * x).sum(0) + w0 * m) / W
        ds = np.where(z > 20.0, 0.0, np.maximum(5.0 * 2.0 ** -23 * s, 2.0 ** -149))
        dw = 2.0 * s * ds + ds * ds
        allow[b] = ((dw * np.abs(x - p)).sum(0) / W + (T + 3) * 2.0 ** -52 * ((w * np.abs(x)).sum(0) + w0 * np.abs(m)) / W
                    + 2.0 ** -24 * np.abs(p))
        phi[b] = p
    return phi, allow


@pytest.mark.parametrize("i", [i for i, c in enumerate(CASES) if c["op"] == XI], ids=[d for d, c in zip(IDS, CASES) if c["op"] == XI])
def test_xi_pool(results, i):
    c = CASES[i]
    status, msg, words = results[i]
    assert status == 0, msg
    B, C, ldo = c["B"], c["C"], c["ldo"]
    words = words.reshape(B + 2, ldo)
    assert (words[0] == FILL).all() and (words[-1] == FILL).all(), "guard row touched"
    assert (words[1:-1, C:] == FILL).all(), "columns past C touched"
    got = words[1:-1, :C].view(np.float32).astype(np.float64)
    assert np.isfinite(got).all()
    want, allow = xi_reference(c)
    ratio = float((np.abs(got - want) / allow).max())
    print(f"max |err| / allowance {ratio:.3f}   max |err| {np.abs(got - want).max():.3e}")
    assert ratio <= 1.0


@pytest.mark.parametrize("i", [i for i, c in enumerate(CASES) if c["op"] == OFFS], ids=[d for d, c in zip(IDS, CASES) if c["op"] == OFFS])
def test_valid_conv_offsets(results, i):
    c = CASES[i]
    status, msg, words = results[i]
    assert status == 0, msg
    B, n = c["B"], len(c["shrinks"])
    assert words[0] == FILL and words[-1] == FILL, "guard word touched"
    got = words[1:-1].view(np.int32).reshape(n, B + 1)
    want = np.stack([c["off"] - np.arange(B + 1, dtype=np.int32) * sh for sh in c["shrinks"]])
    np.testing.assert_array_equal(got, want)
