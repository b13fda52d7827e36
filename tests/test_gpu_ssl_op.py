"""Op-level conformance of the SSL front end's own kernels against float64 (tools/ssl_run).

The runner launches the shipped launchers of libwsp_hip.so (launch_attn, launch_attn_gate,
launch_hubert_pos_conv, launch_layernorm, launch_hubert_conv0) and holds no reference arithmetic; one
run serves all tests.  The references and the element-wise allowances are derived in
tests/ssl_op_ref.py, the cases described in tests/ssl_op_cases.py, and tests/test_ssl_op_ref_cpu.py
shows on the CPU that they tell a faithful kernel from eight wrong ones.  In one line per kernel:
    attention  (2 max_j rel_ij + 2^-16 + (T + 8) 2^-24) sum_j a_ij |v_jd| + 4 * 2^-24 |o_id|,
               rel_ij = (2^-16 + 74 * 2^-24) S_ij + 2 * 2^-24 |g_i table| + 2 * 2^-24 |s_ij - m_i| + E_EXP
    gate       4 f32 ulps of each intermediate + 72 * 2^-24 sum |x| |w| / 4 through each sigmoid + E_GATE / 4
    pos_conv   1.13 ((2^-16 + 6152 * 2^-24) S + 4 * 2^-24 (|y| + |pre|)) + the GELU rule of DESIGN.md section 4
    LayerNorm  |gamma| (rstd dc + |c| dr) + 3 roundings, dc / dr from the kernel's two-pass order
    conv0      1.13 (|scale| 10 * 2^-24 sum |w| |x| + the scale / shift fma) + the GELU rule
Every test also asserts that guard rows, guard columns and rows no utterance owns come back
bit-untouched (NaN pattern 0x7FC5A5A5).  Every attention case runs under pipe 1 and pipe 0, and the
two outputs must agree within the sum of their allowances.

E_EXP / E_GATE are the device's v_exp_f32 / __expf / expf parts: 4 x the largest excess of
|device - float64| over the allowance without them, measured on an MI355X (ceiling 1e-6 relative).
Measured (MI355X, these seeds): no element of any attention or gate case exceeds the allowance
without them, so both excesses are 0 and E_EXP = E_GATE = 0 ship.  max |err| / allowance per case
group, the larger of pipe 1 and pipe 0 where both run:
    attention  lengths .078 (T = 1; .011 .. .039 from T = 31 on), selector .0015, staircases .0062
               (rise .0036, lazy .0062, lazy2 .0036, fall .0014, last .0018), ragged .063, walk .087,
               biased lengths .049 (T = 33; .009 .. .021 from T = 257 on), biased ragged .052, biased
               staircase .152, biased walk .090, zero table .012;  max |err| 5.3e-6
               (walk / biased walk: H = 3 and 94 utterances, 282 items on the 256 CUs: the 26 blocks
               that take a second item all meet another head, 18 of them another length, walk_changes())
    gate       .065 (max |err| 2.6e-7)
    pos_conv   .0041 (max |err| 1.1e-4 on outputs of the utterance filled with 100)
    LayerNorm  random rows .116, offset rows .164 (max |err| 5.7e-3 at mean -300, sd 0.01), constant
               rows 0 (bit-exact beta), featurizer .252
    conv0      random .252, DC offset .124, all-zero utterance .307
The tests found no defect in a kernel.  Three shapes the launchers let through although they would
write or read past a row are now refused by WSP_CHECK and asserted here: attention's ldo < H dh,
LayerNorm's ldx / ldo < D, and an add remap whose last group ends past ldadd.
"""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import op_runner  # noqa: E402
import ssl_op_cases as cases  # noqa: E402
import ssl_op_ref as ref  # noqa: E402
from op_runner import untouched as _untouched  # noqa: E402
from ssl_op_ref import DH, t64  # noqa: E402

pytestmark = pytest.mark.gpu

MEASURED_ATTN_EXCESS = 0.0  # MI355X: largest excess over the allowance without e_exp, relative to 2 sum a |v|
MEASURED_GATE_EXCESS = 0.0  # MI355X: the same for the gate, relative to (|t| + ga |grep|) / 4
E_EXP = 4.0 * MEASURED_ATTN_EXCESS
E_GATE = 4.0 * MEASURED_GATE_EXCESS
assert E_EXP <= 1e-6 and E_GATE <= 1e-6
SINGLES = ("ragged", "walk")  # ragged batches whose utterances also run as batches of one


@pytest.fixture(scope="module")
def res(tmp_path_factory):
    """One runner process for all cases: dict key -> (case, result arrays)."""
    ncu = torch.cuda.get_device_properties(0).multi_processor_count
    todo = []
    for c in cases.attention_cases(ncu):
        for pipe in (1, 0):
            todo.append(((c["name"], pipe), dict(c, pipe=pipe)))
            if c["name"] in SINGLES:
                todo += [((f"{c['name']}[{b}]", pipe), dict(cases.attn_single(c, b), pipe=pipe)) for b in range(c["B"])]
    for c in cases.GATE_CASES + cases.POS_CASES + cases.LN_CASES + cases.CONV0_CASES:
        todo.append((c["name"], c))
    for c, _ in cases.refused_cases():
        todo.append((c["name"], dict(c, pipe=1)))
    assert len(todo) <= 4096 and len({k for k, _ in todo}) == len(todo)
    results = op_runner.run("ssl_run", cases.MAGIC, [cases.op_case(c) for _, c in todo], tmp_path_factory.mktemp("ssl_op"))
    out = {"ncu": ncu}
    for (key, c), r in zip(todo, results):
        out[key] = (c, r)
    return out


def _ran(res, key):
    c, r = res[key]
    assert r["status"] == 0, f"{key} refused: {r['message']}"
    return c, r["arrays"]


def _attn_out(res, name, pipe):
    """The written block [rows][H 64] of an attention case, guards checked."""
    c, (raw,) = _ran(res, (name, pipe))
    raw = raw.reshape(c["rows"] + 8, c["ldo"])
    D = c["H"] * DH
    assert _untouched(raw[c["rows"]:]), f"{name} pipe {pipe}: guard rows written"
    assert _untouched(raw[:c["rows"], D:]), f"{name} pipe {pipe}: guard columns written"
    got = raw[:c["rows"], :D]
    assert np.isfinite(got).all(), f"{name} pipe {pipe}"
    return c, got


_ATTN_REF = {}


def _attn_ref(c):
    if c["name"] not in _ATTN_REF:
        _ATTN_REF[c["name"]] = ref.attn_reference(c)
    return _ATTN_REF[c["name"]]


def _check_attention(res, names):
    """max |err| / allowance per case and pipe, the largest excess over the allowance without E_EXP
    (relative to 2 sum a |v|); both pipes against float64 and against each other."""
    worst, excess = {}, 0.0
    for name in names:
        outs = {}
        for pipe in (1, 0):
            c, got = _attn_out(res, name, pipe)
            want, allow, A = _attn_ref(c)
            err = (t64(got) - want).abs()
            excess = max(excess, float(((err - allow).clamp(min=0) / (2 * A).clamp(min=1e-30)).max()))
            ratio = float((err / (allow + 2 * E_EXP * A)).max())
            worst[(name, pipe)] = ratio
            print(f"\nattn {name} pipe {pipe}: max |err| {float(err.max()):.3e}, |err| / allowance {ratio:.4f}")
            outs[pipe] = t64(got)
        both = float(((outs[1] - outs[0]).abs() / (2 * (allow + 2 * E_EXP * A))).max())
        assert both <= 1.0, f"{name}: pipe 1 and pipe 0 differ by {both:.3f} of the sum of their allowances"
    print(f"\nattn {names[0]} .. {names[-1]}: max |err| / allowance {max(worst.values()):.4f}, excess {excess:.3e}")
    assert 4.0 * excess <= 1e-6, f"device deviation {excess:.3e} is a finding (ceiling 1e-6 / 4)"
    bad = {k: v for k, v in worst.items() if v > 1.0}
    assert not bad, f"|err| / allowance above 1: {bad}"
    return max(worst.values())


def test_attention_lengths(res):
    assert _check_attention(res, [f"len{T}" for T in cases.PLAIN_LENGTHS]) > 0.0


def test_attention_selector(res):
    _check_attention(res, ["selector"])
    pi = cases.selector_perm()
    for pipe in (1, 0):
        c, got = _attn_out(res, "selector", pipe)
        _, allow, _ = _attn_ref(c)
        v = t64(c["qkv"])[:, 2 * c["H"] * DH:3 * c["H"] * DH]
        assert ((t64(got) - v[pi]).abs() <= allow).all(), f"pipe {pipe}: the output is not v[pi(i)]"


def test_attention_staircases(res):
    _check_attention(res, ["stair_rise", "stair_lazy", "stair_lazy2", "stair_fall", "stair_last"])


def test_attention_ragged(res):
    _check_attention(res, ["ragged", "walk"])
    # blocks of the persistent kernel walk more than one item on this device, and between two
    # consecutive items some change head and some change between a 33-frame and a 1-frame utterance
    c, _ = _ran(res, ("walk", 1))
    heads, lens = cases.walk_changes(c, res["ncu"])
    assert heads >= 8 and lens >= 8, f"walk on {res['ncu']} CUs: {heads} head / {lens} length changes"
    for name in SINGLES:
        for pipe in (1, 0):
            c, got = _attn_out(res, name, pipe)
            for b in range(c["B"]):
                _, one = _attn_out(res, f"{name}[{b}]", pipe)
                r0, r1 = int(c["seg"][b]), int(c["seg"][b + 1])
                assert np.array_equal(got[r0:r1].view(np.uint32), one.view(np.uint32)), \
                    f"{name} pipe {pipe}: utterance {b} differs from its batch of one"


def test_attention_biased(res):
    _check_attention(res, [f"bias{T}" for T in cases.BIAS_LENGTHS] + ["bias_ragged", "stair_brise"])
    # the biased walk: a block's next item has another head, so another table in LDS
    _check_attention(res, ["bias_walk"])
    c, _ = _ran(res, ("bias_walk", 1))
    heads, lens = cases.walk_changes(c, res["ncu"])
    assert heads >= 8 and lens >= 8, f"bias_walk on {res['ncu']} CUs: {heads} head / {lens} length changes"


def test_attention_zero_table(res):
    _check_attention(res, ["zero_table"])
    _, plain0 = _attn_out(res, "len257", 0)
    _, zero0 = _attn_out(res, "zero_table", 0)
    assert np.array_equal(plain0.view(np.uint32), zero0.view(np.uint32))  # fma(g, 0, s) = s
    c, plain1 = _attn_out(res, "len257", 1)
    _, zero1 = _attn_out(res, "zero_table", 1)
    _, allow, A = _attn_ref(c)
    assert ((t64(plain1) - t64(zero1)).abs() <= 2 * (allow + 2 * E_EXP * A)).all()


def test_gate(res):
    worst = excess = 0.0
    for g in cases.GATE_CASES:
        c, (raw,) = _ran(res, g["name"])
        raw = raw.reshape(c["rows"] + 8, c["H"])
        assert _untouched(raw[c["rows"]:]), f"{c['name']}: guard rows written"
        got = t64(raw[:c["rows"]])
        assert torch.isfinite(got).all()
        want, allow0, _ = ref.gate_reference(c, 0.0)
        unit = ref.gate_reference(c, 1.0)[1] - allow0  # (|t| + ga |grep|) / 4: the allowance is linear in e_gate
        err = (got - want).abs()
        excess = max(excess, float(((err - allow0).clamp(min=0) / unit).max()))
        ratio = float((err / (allow0 + E_GATE * unit)).max())
        worst = max(worst, ratio)
        print(f"\n{c['name']}: max |err| {float(err.max()):.3e}, |err| / allowance {ratio:.4f}")
    print(f"\ngate: max |err| / allowance {worst:.4f}, excess {excess:.3e}")
    assert 4.0 * excess <= 1e-6, f"device deviation {excess:.3e} is a finding (ceiling 1e-6 / 4)"
    assert 0.0 < worst <= 1.0


def test_pos_conv(res):
    worst = 0.0
    for p in cases.POS_CASES:
        c, (raw,) = _ran(res, p["name"])
        M, gout = c["M"], c["gout"]
        raw = raw.reshape(M + 8, c["ldo"])
        assert _untouched(raw[M:]), f"{c['name']}: guard rows written"
        assert _untouched(raw[:M, 16 * gout:]), f"{c['name']}: guard columns written"
        grp = raw[:M, :16 * gout].reshape(M, 16, gout)
        # the kernel computes 48 of a group's 64 columns and leaves the 16 padding columns alone
        assert _untouched(grp[:, :, 48:]), f"{c['name']}: padding columns written"
        got = t64(grp[:, :, :48])
        assert torch.isfinite(got).all(), c["name"]
        want, allow = ref.pos_conv_reference(c)
        ratio = float(((got - want).abs() / allow).max())
        worst = max(worst, ratio)
        print(f"\n{c['name']}: max |err| {float((got - want).abs().max()):.3e}, |err| / allowance {ratio:.4f}")
    print(f"\npos_conv: max |err| / allowance {worst:.4f}")
    assert 0.0 < worst <= 1.0


def test_layernorm(res):
    worst, worst_feat = {}, 0.0
    for l in cases.LN_CASES:
        c, arrs = _ran(res, l["name"])
        M, D = c["M"], c["D"]
        raw = arrs[0].reshape(M + 8, c["ldo"])
        assert _untouched(raw[M:]) and _untouched(raw[:M, D:]), f"{c['name']}: guards written"
        r = ref.ln_reference(c)
        got = t64(raw[:M, :D])
        assert torch.isfinite(got).all(), c["name"]
        ratio = float(((got - r["out"]).abs() / r["allow"]).max())
        worst[c["kind"]] = max(worst.get(c["kind"], 0.0), ratio)
        print(f"\n{c['name']}: max |err| {float((got - r['out']).abs().max()):.3e}, |err| / allowance {ratio:.4f}")
        assert ratio <= 1.0, c["name"]
        if c["feat_w"] is not None:
            f = arrs[1].reshape(c["frows"] + 8, D)
            assert _untouched(f[c["frows"]:]), f"{c['name']}: feature guard rows written"
            assert bool(r["written"].all())  # every feature row belongs to an utterance
            fr = float(((t64(f[:c["frows"]]) - r["feat"]).abs() / r["dfeat"]).max())
            worst_feat = max(worst_feat, fr)
            assert fr <= 1.0, f"{c['name']}: featurizer |err| / allowance = {fr:.3f}"
        else:
            assert len(arrs) == 1
    print(f"\nlayernorm: max |err| / allowance {worst}, featurizer {worst_feat:.4f}")
    assert set(worst) == {"random", "offset", "constant"} and worst_feat > 0.0


def test_conv0(res):
    worst = {}
    for k in cases.CONV0_CASES:
        c, (raw,) = _ran(res, k["name"])
        raw = raw.reshape(c["orows"] + 8, 512)
        assert _untouched(raw[c["orows"]:]), f"{c['name']}: guard rows written"
        got = t64(raw[:c["orows"]])
        assert torch.isfinite(got).all(), c["name"]
        want, allow = ref.conv0_reference(c)
        ratio = float(((got - want).abs() / allow).max())
        worst[c["kind"]] = max(worst.get(c["kind"], 0.0), ratio)
        print(f"\n{c['name']}: max |err| {float((got - want).abs().max()):.3e}, |err| / allowance {ratio:.4f}")
        assert ratio <= 1.0, c["name"]
    print(f"\nconv0: max |err| / allowance {worst}")
    assert set(worst) == {"random", "dc", "zero"}


def test_refused_shapes(res):
    for c, text in cases.refused_cases():
        _, r = res[c["name"]]
        assert r["status"] == 1 and text in r["message"], f"{c['name']}: {r}"
