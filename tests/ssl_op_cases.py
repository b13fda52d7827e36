"""Cases of the SSL front end's op-level conformance tests (tests/test_gpu_ssl_op.py on the MI355X,
tests/test_ssl_op_ref_cpu.py against the numpy emulations), and their header ints and arrays as the op
table of tools/ssl_run.cpp lists them (`_hdr_arrays`; the file format is tests/op_runner.py's, with 16 header ints).

Attention: H = 2 unless stated, dh = 64, ldq = 3 H 64 + 8 and ldo = H 64 + 4, so strides differ
from widths; the pad columns of qkv are random.  Uniform batches travel without `seg`, ragged ones
with it.  The staircases put the per-chunk key maxima under control: q = [alpha_i, beta_i, noise],
k = [f(j), 1, noise] gives s_ij = (alpha_i f(j) + beta_i) / 8 + noise with |noise| < 0.2 natural
units, f = the key's 32-key chunk (or an indicator of the last key); v carries a per-key offset.
  rise   chunk maxima rise by 12 log2 units per chunk for even queries, by 3 for odd ones
  lazy   chunk maxima rise by 7.6 log2 units over the 10 chunks: no rise over a row's first chunk
         exceeds 8, so the lazy maximum never moves again, and weights reach 2^7 .. 2^8.  (A rise of
         6 per chunk throughout would raise the maximum at the third chunk; the lazy path is what
         this case is for.)
  lazy2  the same 7.6 reached within two chunks (0, 3.8, 7.6, then flat): eight chunks of weights
         near 2^7.6 accumulate on the maximum of the first chunk
  fall   chunk maxima fall by 12 log2 units per chunk: later weights underflow
  last   flat at -40 with the single maximum (+20) in the last live key of the partial chunk
  brise  `rise` with flat q k and the bias supplying it: table linear in j - i, gate 2 / 0.5
"""
import numpy as np

from ssl_op_ref import DH, REL_N, REL_STRIDE, rand_a, rand_w

MAGIC = 0x53505357
OP_ATTN, OP_GATE, OP_POS, OP_LN, OP_CONV0 = 1, 2, 3, 4, 5
LN2 = float(np.log(2.0))
SELECTOR_T = 257


def selector_perm(T=SELECTOR_T):
    """pi(i) = 100 i + 37 mod 257: moves keys inside 32-key chunks, across the 128 / 256
    boundaries and onto the last key (asserted by tests/test_ssl_op_ref_cpu.py)."""
    return (100 * np.arange(T) + 37) % T


# ------------------------------------------------------------------------- attention --
def _attn_pack(name, lens, H, q, k, v, rng, table=None, gate=None, uniform=None, kind="random"):
    """q / k / v [rows][H][64] -> the qkv buffer [rows][3 H 64 + 8]."""
    rows = int(sum(lens))
    D = H * DH
    ldq, ldo = 3 * D + 8, D + 4
    qkv = rand_a(rng, rows, ldq)
    for j, x in enumerate((q, k, v)):
        qkv[:, j * D:(j + 1) * D] = x.reshape(rows, D)
    seg = np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
    if uniform is None:
        uniform = len(set(lens)) == 1
    return dict(op=OP_ATTN, name=name, kind=kind, lens=list(lens), B=len(lens), T=int(max(lens)), H=H, ldq=ldq, ldo=ldo,
                rows=rows, seg=seg, uniform=uniform, qkv=qkv, table=table, gate=gate)


def rand_table(rng, H):
    """Random in [-2, 2] with distinct end values; the 3 pad floats of a head are zero."""
    t = np.zeros((H, REL_STRIDE), np.float32)
    t[:, :REL_N] = rng.uniform(-2.0, 2.0, (H, REL_N))
    t[:, 0], t[:, REL_N - 1] = 1.75, -1.25
    return t


def attn_random(name, lens, seed, H=2, bias=False, zero_table=False, uniform=None):
    rng = np.random.default_rng(seed)
    rows = int(sum(lens))
    q, k, v = (rand_a(rng, rows, H * DH).reshape(rows, H, DH) for _ in range(3))
    table = gate = None
    if bias or zero_table:
        table = rand_table(rng, H)
        gate = rng.uniform(0.5, 2.5, (rows, H)).astype(np.float32)
        if zero_table:
            table[:] = 0.0
    return _attn_pack(name, lens, H, q, k, v, rng, table, gate, uniform)


def attn_selector(seed=301, H=2):
    """q_i = c k_pi(i) with k random signs: the score of key pi(i) exceeds all others by >= 60."""
    rng = np.random.default_rng(seed)
    T = SELECTOR_T
    pi = selector_perm()
    k = rng.choice(np.array([-1.0, 1.0], np.float32), size=(T, H, DH))
    cross = np.einsum("ihd,jhd->hij", k, k)
    cross[:, np.arange(T), np.arange(T)] = -DH
    c = np.float32(np.ceil(61.0 * 8.0 / (DH - cross.max()) * 4.0) / 4.0)  # margin 61: 60 holds in any rounding
    q = c * k[pi]
    v = rand_a(rng, T, H * DH).reshape(T, H, DH)
    return _attn_pack("selector", [T], H, q, k, v, rng, kind="selector")


def attn_staircase(variant, seed, T=300, H=2):
    rng = np.random.default_rng(seed)
    amp = np.float32(0.3)
    q, k = (amp * rand_a(rng, T, H * DH).reshape(T, H, DH) for _ in range(2))
    j = np.arange(T)
    chunk, nch = (j // 32).astype(np.float32), (T + 31) // 32
    odd = (j % 2 == 1)[:, None]
    table = gate = None
    k[:, :, 1] = 1.0
    if variant in ("rise", "lazy", "fall"):
        per = {"rise": np.where(odd, 3.0, 12.0), "lazy": np.full((T, 1), 7.6 / (nch - 1)),
               "fall": np.full((T, 1), -12.0)}[variant] * LN2  # natural units per chunk
        k[:, :, 0] = chunk[:, None]
        q[:, :, 0] = 8.0 * per
        q[:, :, 1] = -8.0 * per * (nch - 1) / 2  # centred: |score| <= 12 ln 2 * 4.5 + noise < 100
    elif variant == "lazy2":
        k[:, :, 0] = np.minimum(chunk, 2.0)[:, None]
        q[:, :, 0], q[:, :, 1] = 8.0 * 3.8 * LN2, -8.0 * 3.8 * LN2
    elif variant == "last":
        k[:, :, 0] = (j == T - 1)[:, None]
        q[:, :, 0], q[:, :, 1] = 8.0 * 60.0, -8.0 * 40.0
    else:  # brise: q . k is noise only; the bias g_i table[j - i] rises by 12 / 3 log2 units per 32 keys
        assert variant == "brise"
        q[:, :, :2] = 0.0
        table = rand_table(rng, H)
        d = np.arange(-T + 1, T)
        table[:, d + (REL_N - 1) // 2] = (6.0 * LN2 / 32.0 * d).astype(np.float32)
        gate = np.where(odd, 0.5, 2.0).astype(np.float32).repeat(H, axis=1)
    off = ((j * 37) % 101 / 50.0 - 1.0).astype(np.float32)  # per-key offset: a wrong weight shows
    v = np.float32(0.1) * rand_a(rng, T, H * DH).reshape(T, H, DH) + off[:, None, None]
    return _attn_pack("stair_" + variant, [T], H, q.astype(np.float32), k.astype(np.float32), v, rng, table, gate,
                      kind=variant)


PLAIN_LENGTHS = [1, 31, 32, 33, 127, 128, 129, 255, 256, 257, 300]
BIAS_LENGTHS = [33, 257, 768, 769, 800, 1000]
RAGGED = [1, 129, 257, 40, 300]


def walk_shape(ncu):
    """(H, B) of the walk batches (lengths alternating 33 / 1, one query block): ncu + 24 items or a
    few more, so 24 blocks of the persistent kernel take a second item `ncu` further on, and H not
    dividing ncu, so that item has another head; walk_changes() counts what the blocks meet."""
    H = next(h for h in (2, 3, 5, 7) if ncu % h)
    return H, (ncu + 24 + H - 1) // H


def walk_changes(c, ncu):
    """The item walk of attn_pipe_kernel over case c on `ncu` CUs, restated: block x takes items x,
    x + grid, ... with grid = min(items, ncu), item = (utterance H + head) nqb + query block, and
    skips items with no queries in their block.  Returns (blocks that change head between two
    consecutive items, blocks that change utterance length)."""
    H, nqb = c["H"], (c["T"] + 255) // 256
    n = c["B"] * H * nqb
    grid = min(n, ncu)
    heads = lens = 0
    for x in range(grid):
        its = [it for it in range(x, n, grid) if (it % nqb) * 256 < c["lens"][it // (H * nqb)]]
        pairs = list(zip(its, its[1:]))
        heads += any((a // nqb) % H != (b // nqb) % H for a, b in pairs)
        lens += any(c["lens"][a // (H * nqb)] != c["lens"][b // (H * nqb)] for a, b in pairs)
    return heads, lens


def attention_cases(ncu):
    """Every attention case but the batch-of-one twins; `ncu` = the device's CU count (the CPU tests
    pass a small one and the MI355X's 256)."""
    cs = [attn_random(f"len{T}", [T, T], 100 + T) for T in PLAIN_LENGTHS]
    cs.append(attn_selector())
    cs += [attn_staircase(v, 310 + i) for i, v in enumerate(("rise", "lazy", "fall", "last"))]
    cs.append(attn_staircase("lazy2", 315))
    cs.append(attn_random("ragged", RAGGED, 320))
    H, B = walk_shape(ncu)
    walk_lens = [33 if b % 2 == 0 else 1 for b in range(B)]
    cs.append(attn_random("walk", walk_lens, 321, H=H))
    cs.append(attn_random("bias_walk", walk_lens, 322, H=H, bias=True))  # the table hand-over at a head change
    cs += [attn_random(f"bias{T}", [T], 400 + T, bias=True) for T in BIAS_LENGTHS]
    cs.append(attn_random("bias_ragged", [800, 33], 330, bias=True))
    cs.append(attn_staircase("brise", 331))
    cs.append(attn_random("zero_table", [257, 257], 100 + 257, zero_table=True))  # len257's q / k / v
    return cs


def attn_single(c, b):
    """Utterance b of a ragged case as a batch of one (the same rows, bit for bit)."""
    r0, r1 = int(c["seg"][b]), int(c["seg"][b + 1])
    s = dict(c, name=f"{c['name']}[{b}]", lens=[r1 - r0], B=1, T=r1 - r0, rows=r1 - r0, uniform=True,
             seg=np.array([0, r1 - r0], np.int32), qkv=c["qkv"][r0:r1])
    if c["gate"] is not None:
        s["gate"] = c["gate"][r0:r1]
    return s


# ------------------------------------------------------------------------------ gate --
def gate_case(seed, rows, H):
    rng = np.random.default_rng(seed)
    ldx = H * DH + 4
    w = np.concatenate([rand_w(rng, 2 * DH, amp=1.5), rand_w(rng, 2, amp=1.0), rng.uniform(0.5, 1.5, H).astype(np.float32)])
    x = rand_a(rng, rows, ldx)
    # each dot product's weights and bias scaled so that its largest |argument| over the case is 12
    xh = x[:, :H * DH].astype(np.float64).reshape(rows, H, DH)
    for j in range(2):
        arg = xh @ w[j * DH:(j + 1) * DH].astype(np.float64) + float(w[2 * DH + j])
        f = np.float32(12.0 / np.abs(arg).max() * (1.0 - 1e-6))
        w[j * DH:(j + 1) * DH] *= f
        w[2 * DH + j] *= f
    return dict(op=OP_GATE, name=f"gate{rows}x{H}", rows=rows, H=H, ldx=ldx, x=x, w=w)


GATE_CASES = [gate_case(500 + 16 * i + H, rows, H) for i, rows in enumerate((1, 5, 300)) for H in (1, 12)]


# -------------------------------------------------------------------------- pos_conv --
def pos_case(seed, lens, hot=None):
    """`hot`: an utterance filled with 100 (its neighbours must not read it)."""
    rng = np.random.default_rng(seed)
    M, gout, ldx, ldo = int(sum(lens)), 64, 768 + 8, 1024 + 16
    seg = np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
    x = rand_a(rng, M, ldx)
    if hot is not None:
        x[seg[hot]:seg[hot + 1]] = 100.0
    w = rand_w(rng, 16, gout, 48, 128, amp=0.02)
    w[:, 48:] = 0.0  # the padded grouped weight: rows 48..63 of a group are zero
    bias = rand_w(rng, 16, gout, amp=0.3)
    bias[:, 48:] = 0.0
    return dict(op=OP_POS, name=f"pos{lens}", lens=list(lens), B=len(lens), maxT=int(max(lens)), M=M, ldx=ldx, ldo=ldo,
                gout=gout, seg=seg, x=x, w=w.reshape(16 * gout, 48, 128), bias=bias.reshape(-1))


POS_CASES = [pos_case(601, [1]), pos_case(602, [63, 64, 65]), pos_case(603, [255, 256, 257]),
             pos_case(604, [300, 2, 129], hot=1)]


# ------------------------------------------------------------------------- LayerNorm --
def ln_case(seed, M, D, add=False, kind="random", feat=None, lens=None, flens=None, name=None):
    """feat = (feat_init, T, Tout) for a uniform featurizer, (feat_init,) with lens / flens for a
    segmented one."""
    rng = np.random.default_rng(seed)
    ldx, ldo = D + 8, D + 4
    x = rand_a(rng, M, ldx) * np.float32(2.0)
    if kind == "offset":  # |mean| far above the standard deviation (outlier channels)
        x = rng.standard_normal((M, ldx)).astype(np.float32)
        x[0::2] = x[0::2] + np.float32(100.0)
        x[1::2] = x[1::2] * np.float32(0.01) - np.float32(300.0)
    elif kind == "constant":
        x[:, :D] = np.float32(3.0) + np.arange(M, dtype=np.float32)[:, None]
    c = dict(op=OP_LN, name=name or f"ln{M}x{D}{'+add' if add else ''}_{kind}", M=M, D=D, ldx=ldx, ldo=ldo, x=x, add=None,
             ldadd=0, gin=0, gout=0, gamma=(1.0 + rand_w(rng, D, amp=0.5)).astype(np.float32), beta=rand_w(rng, D, amp=0.5),
             eps=1e-5, feat_w=None, feat_init=0, T=0, Tout=0, seg=None, fseg=None, frows=0, prior=None, kind=kind)
    if add:
        c.update(ldadd=1024, gin=48, gout=64, add=rand_a(rng, M, 1024))
    if feat is not None:
        c["feat_w"], c["feat_init"] = np.float32(0.37), feat[0]
        if lens is None:
            c["T"], c["Tout"] = feat[1], feat[2]
            c["frows"] = M // feat[1] * feat[2]
        else:
            c["seg"] = np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
            c["fseg"] = np.concatenate([[0], np.cumsum(flens)]).astype(np.int32)
            c["frows"] = int(sum(flens))
        if not feat[0]:
            c["prior"] = rand_a(rng, c["frows"], D)
    return c


LN_CASES = (
    [ln_case(700 + 10 * i + M, M, D, add) for i, (D, add) in enumerate(((512, False), (768, False), (512, True), (768, True)))
     for M in (1, 4, 5, 9)]
    + [ln_case(750 + D, 6, D, kind="offset") for D in (512, 768)]
    + [ln_case(760 + D, 3, D, kind="constant") for D in (512, 768)]
    + [ln_case(770, 10, 768, add=True, feat=(1, 5, 6), name="feat_init_grow"),
       ln_case(771, 10, 768, feat=(0, 5, 6), name="feat_acc_grow"),
       ln_case(772, 10, 768, feat=(0, 5, 4), name="feat_acc_trim"),
       ln_case(773, 10, 512, feat=(1, 5, 5), name="feat_init_same"),
       ln_case(774, 9, 768, feat=(1,), lens=[3, 1, 5], flens=[4, 1, 4], name="feat_init_seg"),
       ln_case(775, 9, 768, add=True, feat=(0,), lens=[3, 1, 5], flens=[4, 1, 4], name="feat_acc_seg")])


# ----------------------------------------------------------------------------- conv0 --
def conv0_case(seed, lens, kind="random", segmented=False):
    rng = np.random.default_rng(seed)
    utts = []
    for i, N in enumerate(lens):
        x = rng.uniform(-1.0, 1.0, N).astype(np.float32)
        if kind == "dc":  # DC offset 0.5, amplitude 1e-3
            x = (np.float32(0.5) + np.float32(1e-3) * x).astype(np.float32)
        elif kind == "zero" and i == 0:
            x[:] = 0.0
        utts.append(x)
    T0s = [(N - 10) // 5 + 1 for N in lens]
    c = dict(op=OP_CONV0, name=f"conv0{lens}_{kind}{'_seg' if segmented else ''}", B=len(lens), lens=list(lens), T0s=T0s,
             T0=max(T0s), utts=utts, w=rand_w(rng, 512, 10, amp=0.3), gamma=(1.0 + rand_w(rng, 512, amp=0.5)).astype(np.float32),
             beta=rand_w(rng, 512, amp=0.5), segmented=segmented, kind=kind, orows=int(sum(T0s)))
    if segmented:
        c["wav"] = np.concatenate(utts)
        c["wseg"] = np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
        c["oseg"] = np.concatenate([[0], np.cumsum(T0s)]).astype(np.int32)
        c["N"] = c["ldw"] = 0
    else:
        assert len(set(lens)) == 1
        c["N"], c["ldw"] = lens[0], lens[0] + 3  # a row stride above the length
        wav = rng.uniform(-1.0, 1.0, (len(lens), c["ldw"])).astype(np.float32)
        for i, x in enumerate(utts):
            wav[i, :lens[0]] = x
        c["wav"] = wav.reshape(-1)
    return c


CONV0_CASES = ([conv0_case(800 + i, [N, N]) for i, N in enumerate((10, 14, 15, 400, 5130, 5135))]
               + [conv0_case(810, [5135, 5135], kind="dc"), conv0_case(811, [400, 400], kind="zero"),
                  conv0_case(812, [400, 10, 5135], segmented=True)])


# ---------------------------------------------------------------------- refused shapes --
def refused_cases():
    """Shapes the launchers refuse by WSP_CHECK: (case, the refusal's text)."""
    a = attn_random("refuse_dh", [5], 900)
    ln = ln_case(901, 2, 768, add=True)
    c0 = dict(conv0_case(902, [400, 400]), name="refuse_T0")
    c0["T0"] = c0["T0"] + 1  # not (N - 10) / 5 + 1
    c0["orows"] = 2 * c0["T0"]
    return [(dict(a, dh=32), "head dim must be 64"),
            (dict(a, name="refuse_ldo", ldo=64), "attn: bad shape"),  # rows of 2 heads would overlap
            (dict(ln_case(903, 2, 640), name="refuse_D"), "D must be 512 or 768"),
            (dict(ln, name="refuse_ldx", ldx=256, x=ln["x"][:, :256]), "rows narrower than D"),
            (dict(ln, name="refuse_ln_ldo", ldo=256), "rows narrower than D"),
            # the last group's 48 channels would end at column 1008 of a 1000-column row
            (dict(ln, name="refuse_ldadd", ldadd=1000, add=ln["add"][:, :1000]), "bad add remap"),
            (c0, "bad frame count")]


# ------------------------------------------------------------- header ints and arrays --
def _hdr_arrays(c):
    op = c["op"]
    if op == OP_ATTN:
        nseg = 0 if c["uniform"] else c["B"]
        hdr = [c["B"], c["T"], c["H"], c.get("dh", DH), c["ldq"], c["ldo"], c["rows"], nseg, c["pipe"],
               int(c["table"] is not None)]
        arrs = [c["qkv"]] + ([c["seg"]] if nseg else []) + ([c["table"], c["gate"]] if c["table"] is not None else [])
    elif op == OP_GATE:
        hdr, arrs = [c["rows"], c["H"], c["ldx"]], [c["x"], c["w"]]
    elif op == OP_POS:
        hdr = [c["B"], c["maxT"], c["M"], c["ldx"], c["ldo"], c["gout"]]
        arrs = [c["x"], c["seg"], c["w"], c["bias"]]
    elif op == OP_LN:
        feat = c["feat_w"] is not None
        nseg = 0 if c["seg"] is None else len(c["seg"]) - 1
        hdr = [c["M"], c["D"], c["ldx"], c["ldo"], int(c["add"] is not None), c["ldadd"], c["gin"], c["gout"], int(feat),
               c["feat_init"], c["T"], c["Tout"], nseg, c["frows"]]
        arrs = ([c["x"]] + ([c["add"]] if c["add"] is not None else [])
                + [c["gamma"], c["beta"], np.array([c["eps"], c["feat_w"] if feat else 0.0], np.float32)]
                + ([c["seg"], c["fseg"]] if nseg else []) + ([c["prior"]] if feat and not c["feat_init"] else []))
    else:
        seg = c["segmented"]
        hdr = [c["B"], c["N"], c["ldw"], c["T0"], c["B"] if seg else 0, c["wav"].size, c["orows"]]
        arrs = [c["wav"], c["w"], c["gamma"], c["beta"]] + ([c["wseg"], c["oseg"]] if seg else [])
    return hdr, arrs


def op_case(c):
    """The case as tests/op_runner.py writes it: (op, header ints, arrays)."""
    return (c["op"], *_hdr_arrays(c))
