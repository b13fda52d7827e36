"""ReDimNetB2 on one GPU: step time, embeddings per second, algorithmic TF/s, the per-class times of
the handle's profiler against each class's HBM floor, and the same model in eager torch for scale.

    python scripts/redimnet_timing.py [--batch 256] [--frames 200] [--repeats 5] [--steps 3] [--eager]
                                      [--opt key=value ...]

The shapes DESIGN.md reports are B = 256 x T = 200 and B = 128 x T = 498.  The HIP path is timed in
`repeats` windows of `steps` forwards between device synchronisations and reported as the median;
--eager adds tests/redimnet_ref.py (torch functional ops, f32) on the same GPU and shape.  The
per-class times come from a run of their own with the profiler on.  A class's HBM floor is the bytes
its launches must move (each operand read once, each result written once, f32; weights not counted)
over 6.3 TB/s, the rate a float4 copy reaches on the MI355X; K / V re-reads of attention and halo
re-reads are not in the floor.  Prints one JSON line (development tool, not part of the bench
contract)."""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import time

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))
import redimnet_ref  # noqa: E402
from wespeaker_hubert_amd.arch import redimnet_gflop_per_utt, redimnet_stage_dims  # noqa: E402
from wespeaker_hubert_amd.speaker_model import HipSpeakerModel  # noqa: E402
from wespeaker_hubert_amd.synthetic import synth_feats, synth_state_dict  # noqa: E402

ARCH = "ReDimNetB2"
HBM_TBS = 6.3  # the achievable HBM rate the rooflines in DESIGN.md use
D = 1152


def floors_floats(M):
    """f32 values each class must move per step over M = B * T frame rows"""
    st = redimnet_stage_dims(ARCH)
    hs = [d[6] for d in st]
    nblk = sum(d[5] for d in st)
    return {
        "rd_stem": M * (72 + D),
        "rd_entry": sum((si + 2) * M * D for si in range(len(st))),  # si + 1 inputs, one output
        "rd_block2d": nblk * 2 * M * D,
        "rd_red": sum(M * (D + h) for h in hs),
        "rd_ln": sum((2 + 3 + 3) * M * h for h in hs),
        "rd_block1d": sum(4 * 2 * M * h for h in hs),
        "rd_qkv": sum(4 * M * h for h in hs),
        "rd_attn": sum(4 * M * h for h in hs),
        "rd_lin": sum(3 * 2 * M * h for h in hs),
        "rd_gelu": sum(2 * M * h for h in hs),
        "rd_exp": sum(M * (h + 2 * D) for h in hs),  # the skip is read, the stage output written
        "rd_wsum": (len(st) + 2) * M * D,
        "pool_linear1": M * (D + 128),
        "pool_linear2": M * (128 + D),
        "astp": 2 * M * D,
    }


def _timed(f, repeats, steps):
    f()
    torch.cuda.synchronize()
    ts = []
    for _ in range(repeats):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(steps):
            f()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) / steps)
    return statistics.median(ts), min(ts), max(ts)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--frames", type=int, default=200)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--eager", action="store_true")
    ap.add_argument("--opt", action="append", default=[], help="handle option, e.g. precision=0")
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(0)
    B, T, E = a.batch, a.frames, 192
    model = HipSpeakerModel(ARCH, feat_dim=72, embed_dim=E)
    sd = synth_state_dict(87, model.state_dict_layout())
    model.load_state_dict(sd)
    for kv in a.opt:
        k, _, v = kv.partition("=")
        model.set_option(k, int(v))
    model.to(dev)
    feats = torch.from_numpy(synth_feats(7, B, T, 72)).to(dev)
    emb = torch.empty(B, E, device=dev)

    def hip():
        model.embed(feats, out=emb)

    med, lo, hi = _timed(hip, a.repeats, a.steps)
    gf = redimnet_gflop_per_utt(model.spec, T)
    out = {"arch": ARCH, "batch": B, "frames": T, "repeats": a.repeats, "steps": a.steps, "opt": a.opt,
           "gflop_per_utt": round(gf, 3),
           "hip": {"step_ms": round(med * 1e3, 3), "emb_per_s": round(B / med, 1), "tflops": round(gf * B / med / 1e3, 2),
                   "spread_ms": [round(lo * 1e3, 3), round(hi * 1e3, 3)]}}
    if a.eager:
        sd_dev = {k: torch.from_numpy(v).to(dev) for k, v in sd.items() if not k.endswith("num_batches_tracked")}
        eager = lambda: redimnet_ref.forward(feats, sd_dev, ARCH, dtype=torch.float32)  # noqa: E731
        m2, l2, h2 = _timed(eager, a.repeats, a.steps)
        out["eager"] = {"step_ms": round(m2 * 1e3, 3), "emb_per_s": round(B / m2, 1),
                        "spread_ms": [round(l2 * 1e3, 3), round(h2 * 1e3, 3)]}
        out["eager_over_hip"] = round(m2 / med, 3)
        hip()
        out["max_abs_diff_vs_eager"] = float((emb - eager()).abs().max())
    # per-class times, profiler on, in a run of their own
    torch.cuda.synchronize()
    model.profile(True)
    for _ in range(a.steps):
        hip()
    torch.cuda.synchronize()
    model.profile(False)
    classes, total = {}, 0.0
    for t, floats in floors_floats(B * T).items():
        n, ms, fl = model.profile_query(t)
        if n:
            floor_ms = floats * 4 / (HBM_TBS * 1e12) * 1e3
            classes[t] = {"launches_per_step": n // a.steps, "ms_per_step": round(ms / a.steps, 4),
                          "hbm_floor_ms": round(floor_ms, 4), "of_floor": round(ms / a.steps / floor_ms, 2),
                          "tflops": round(fl * n / (ms * 1e-3) / 1e12, 2) if fl else None}
            total += ms / a.steps
    out["classes"] = classes
    out["classes_ms_per_step"] = round(total, 3)
    assert torch.isfinite(emb).all()
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
