"""Gemini DF-ResNet (feat 80 / embed 256) on one GPU: step time, embeddings per second, algorithmic
TF/s, the ib_fused 0 / 1 A/B and the per-class times of the handle's profiler.

    python scripts/gemini_timing.py [--arch Gemini_DF_ResNet114] [--batch 64] [--frames 200] [--repeats 5]
                                    [--steps 3] [--eager] [--opt key=value ...]

The HIP path is timed in `repeats` windows of `steps` forwards between device synchronisations
and reported as the median, once per route ("fused": ib_fused = 1, conv1 + tail; "unfused":
ib_fused = 0, conv1 + depthwise conv + conv3), the routes interleaved inside every repeat; --eager
adds tests/gemini_ref.py (torch functional ops, f32) on the same GPU and shape and compares the
embeddings.  The per-class times come from runs of their own with the profiler on, one per route.
Prints one JSON line (development tool, not part of the bench contract)."""
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
import gemini_ref  # noqa: E402
from wespeaker_hubert_amd.arch import gemini_gflop_per_utt  # noqa: E402
from wespeaker_hubert_amd.speaker_model import HipSpeakerModel  # noqa: E402
from wespeaker_hubert_amd.synthetic import synth_feats, synth_state_dict  # noqa: E402

TAGS = ("stem", "gem_down", "gem_pw1", "gem_dw", "gem_pw2", "gem_tail", "tstp_head")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--arch", default="Gemini_DF_ResNet114")
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--frames", type=int, default=200)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--eager", action="store_true")
    ap.add_argument("--opt", action="append", default=[], help="handle option, e.g. streams=2")
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(0)
    B, T = a.batch, a.frames
    model = HipSpeakerModel(a.arch, feat_dim=80, embed_dim=256)
    sd = synth_state_dict(71, model.state_dict_layout(), residual_tame=True)
    model.load_state_dict(sd)
    for kv in a.opt:
        k, _, v = kv.partition("=")
        model.set_option(k, int(v))
    model.to(dev)
    default = model.get_option("ib_fused")
    feats = torch.from_numpy(synth_feats(7, B, T, 80)).to(dev)
    emb = torch.empty(B, 256, device=dev)

    def hip():
        model.embed(feats, out=emb)

    variants = {"fused": (lambda: model.set_option("ib_fused", 1), hip),
                "unfused": (lambda: model.set_option("ib_fused", 0), hip)}
    if a.eager:
        sd_dev = {k: torch.from_numpy(v).to(dev) for k, v in sd.items() if not k.endswith("num_batches_tracked")}
        variants["eager"] = (lambda: None, lambda: gemini_ref.forward(feats, sd_dev, a.arch))
    for setup, f in variants.values():  # warm up at the timed shape
        setup()
        f()
    torch.cuda.synchronize()
    times = {k: [] for k in variants}
    for _ in range(a.repeats):
        for k, (setup, f) in variants.items():
            setup()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(a.steps):
                f()
            torch.cuda.synchronize()
            times[k].append((time.perf_counter() - t0) / a.steps)
    med = {k: statistics.median(v) for k, v in times.items()}
    gf = gemini_gflop_per_utt(model.spec, T)
    out = {"arch": a.arch, "batch": B, "frames": T, "repeats": a.repeats, "steps": a.steps, "opt": a.opt,
           "ib_fused_default": default, "gflop_per_utt": round(gf, 3)}
    for k, v in med.items():
        out[k] = {"step_ms": round(v * 1e3, 3), "emb_per_s": round(B / v, 1),
                  "spread_ms": [round(min(times[k]) * 1e3, 3), round(max(times[k]) * 1e3, 3)]}
        if k != "eager":
            out[k]["tflops"] = round(gf * B / v / 1e3, 2)
    out["unfused_over_fused"] = round(med["unfused"] / med["fused"], 3)
    embs = {}
    for k in ("fused", "unfused"):
        variants[k][0]()
        hip()
        embs[k] = emb.clone()
    out["max_abs_diff_fused_vs_unfused"] = float((embs["fused"] - embs["unfused"]).abs().max())
    if a.eager:
        out["fused_over_eager"] = round(med["eager"] / med["fused"], 3)
        out["max_abs_diff_vs_eager"] = float((embs["fused"] - variants["eager"][1]()).abs().max())
    # per-class times, profiler on, in runs of their own
    out["classes"] = {}
    for k in ("fused", "unfused"):
        variants[k][0]()
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
        out["classes"][k] = classes
    model.set_option("ib_fused", default)
    assert torch.isfinite(emb).all()
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
