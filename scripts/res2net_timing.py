"""Res2Net (feat 80 / embed 256) on one GPU: step time, embeddings per second, algorithmic TF/s, the
per-class times of the handle's profiler and, per stage, the time of the block tail under the
schedule the handle runs (option res2_tail: 0 = 3x3 conv + conv3 over the concatenated operand,
2 = the fused tail in every stage, 1 = the shipped per-stage choice).

    python scripts/res2net_timing.py [--arch Res2Net34_Base] [--batch 64] [--frames 200] [--repeats 5]
                                     [--steps 3] [--eager] [--opt key=value ...]

The HIP path is timed in `repeats` windows of `steps` forwards between device synchronisations
and reported as the median; --eager adds tests/res2net_ref.py (torch functional ops, f32) on the
same GPU and shape and compares the embeddings.  The per-class times come from a run of their own
with the profiler on; `tail_ms` sums, per stage, the classes of the tail (res2_conv3x3 + res2_pw.c3,
or res2_tail).  `max_abs_diff_fused_vs_unfused` compares the embeddings of res2_tail = 2 and 0 in this
process.  Prints one JSON line (development tool, not part of the bench contract)."""
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
import res2net_ref  # noqa: E402
from wespeaker_hubert_amd.arch import res2net_gflop_per_utt  # noqa: E402
from wespeaker_hubert_amd.speaker_model import HipSpeakerModel  # noqa: E402
from wespeaker_hubert_amd.synthetic import synth_feats, synth_state_dict  # noqa: E402

TAGS = ("stem", "res2_pw.c1", "res2_pw.sc", "res2_conv3x3", "res2_pw.c3", "res2_tail", "tstp_head")
TAIL_TAGS = ("res2_conv3x3", "res2_pw.c3", "res2_tail")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--arch", default="Res2Net34_Base")
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--frames", type=int, default=200)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--eager", action="store_true")
    ap.add_argument("--opt", action="append", default=[], help="handle option, e.g. res2_tail=0")
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(0)
    B, T = a.batch, a.frames
    model = HipSpeakerModel(a.arch, feat_dim=80, embed_dim=256)
    sd = synth_state_dict(171, model.state_dict_layout(), residual_tame=True)
    model.load_state_dict(sd)
    for kv in a.opt:
        k, _, v = kv.partition("=")
        model.set_option(k, int(v))
    model.to(dev)
    feats = torch.from_numpy(synth_feats(7, B, T, 80)).to(dev)
    emb = torch.empty(B, 256, device=dev)

    def hip():
        model.embed(feats, out=emb)

    variants = {"hip": hip}
    if a.eager:
        sd_dev = {k: torch.from_numpy(v).to(dev) for k, v in sd.items() if not k.endswith("num_batches_tracked")}
        variants["eager"] = lambda: res2net_ref.forward(feats, sd_dev, a.arch)
    for f in variants.values():  # warm up at the timed shape
        f()
    torch.cuda.synchronize()
    times = {k: [] for k in variants}
    for _ in range(a.repeats):
        for k, f in variants.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(a.steps):
                f()
            torch.cuda.synchronize()
            times[k].append((time.perf_counter() - t0) / a.steps)
    med = {k: statistics.median(v) for k, v in times.items()}
    out = {"arch": a.arch, "batch": B, "frames": T, "repeats": a.repeats, "steps": a.steps, "opt": a.opt,
           "res2_tail": model.get_option("res2_tail")}
    for k, v in med.items():
        out[k] = {"step_ms": round(v * 1e3, 3), "emb_per_s": round(B / v, 1),
                  "spread_ms": [round(min(times[k]) * 1e3, 3), round(max(times[k]) * 1e3, 3)]}
    gf = res2net_gflop_per_utt(model.spec, T)
    out["gflop_per_utt"] = round(gf, 3)
    out["hip"]["tflops"] = round(gf * B / med["hip"] / 1e3, 2)
    hip()
    if a.eager:
        out["hip_over_eager"] = round(med["eager"] / med["hip"], 3)
        out["max_abs_diff_vs_eager"] = float((emb - variants["eager"]()).abs().max())
    # per-class times, profiler on, in a run of its own
    torch.cuda.synchronize()
    model.profile(True)
    for _ in range(a.steps):
        hip()
    torch.cuda.synchronize()
    model.profile(False)
    classes = {}
    for t in TAGS:
        n, ms, fl = model.profile_query(t)
        if n:
            classes[t] = {"launches_per_step": n // a.steps, "ms_per_step": round(ms / a.steps, 4),
                          "tflops": round(fl * n / (ms * 1e-3) / 1e12, 2) if fl else None}
    out["classes"] = classes
    # the block tail per stage: the classes carry the stage as ".L<n>"
    out["tail_ms"] = {f"L{li}": round(sum(model.profile_query(f"{t}.L{li}")[1] for t in TAIL_TAGS) / a.steps, 4)
                      for li in (1, 2, 3, 4)}
    keep = model.get_option("res2_tail")
    both = {}
    for v in (2, 0):
        model.set_option("res2_tail", v)
        both[v] = model.embed(feats).clone()
    model.set_option("res2_tail", keep)
    out["max_abs_diff_fused_vs_unfused"] = float((both[2] - both[0]).abs().max())
    assert torch.isfinite(emb).all()
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
