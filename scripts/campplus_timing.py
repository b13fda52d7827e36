"""CAM++ (CAMPPlus, feat 80 / embed 512) at B = 256 x T = 498 frames on one GPU.

    python scripts/campplus_timing.py [--batch 256] [--frames 498] [--repeats 5] [--steps 3] [--no-eager]
                                      [--opt key=value ...]

Three variants are timed in interleaved repeats (A B C A B C ..., each repeat `steps` forwards
between device synchronisations) and reported as medians:
  hip        the HIP path, default options (BN-ReLU inside the dense GEMMs' A prologue)
  unfused    the same with option cam_fused = 0 (the BN-ReLU as an elementwise pass of its own)
  eager      tests/campplus_ref.py (torch functional ops, f32) on the same GPU and shape
then, in a run of its own, the HIP path's per-class times from the handle's profiler and the
achieved TF/s from arch.campplus_gflop_per_utt.  The HIP and eager embeddings of the timed shape
are compared.  Prints one JSON line (development tool, not part of the bench contract)."""
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
import campplus_ref  # noqa: E402
from wespeaker_hubert_amd.arch import campplus_gflop_per_utt  # noqa: E402
from wespeaker_hubert_amd.speaker_model import HipSpeakerModel  # noqa: E402
from wespeaker_hubert_amd.synthetic import synth_feats, synth_state_dict  # noqa: E402

TAGS = ("stem", "fcm_strided", "fcm_conv3x3", "cam_tdnn", "cam_gemm", "cam_mask", "cam_local", "cam_transit",
        "cam_bnrelu", "tstp_head")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--frames", type=int, default=498)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--no-eager", action="store_true")
    ap.add_argument("--opt", action="append", default=[], help="handle option, e.g. streams=2")
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(0)
    B, T = a.batch, a.frames
    model = HipSpeakerModel("CAMPPlus", feat_dim=80, embed_dim=512)
    sd = synth_state_dict(41, model.state_dict_layout())
    model.load_state_dict(sd)
    for kv in a.opt:
        k, _, v = kv.partition("=")
        model.set_option(k, int(v))
    model.to(dev)
    feats = torch.from_numpy(synth_feats(7, B, T, 80)).to(dev)
    emb = torch.empty(B, 512, device=dev)
    sd_dev = {k: torch.from_numpy(v).to(dev) for k, v in sd.items() if not k.endswith("num_batches_tracked")}

    def hip():
        model.embed(feats, out=emb)

    # name -> (set-up outside the timed window, the timed forward)
    variants = {"hip": (lambda: model.set_option("cam_fused", 1), hip),
                "unfused": (lambda: model.set_option("cam_fused", 0), hip)}
    if not a.no_eager:
        variants["eager"] = (lambda: None, lambda: campplus_ref.forward(feats, sd_dev))
    for pre, f in variants.values():  # warm up every variant at the timed shape
        pre()
        f()
    torch.cuda.synchronize()
    times = {k: [] for k in variants}
    for _ in range(a.repeats):
        for k, (pre, f) in variants.items():
            pre()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(a.steps):
                f()
            torch.cuda.synchronize()
            times[k].append((time.perf_counter() - t0) / a.steps)
    med = {k: statistics.median(v) for k, v in times.items()}
    out = {"batch": B, "frames": T, "repeats": a.repeats, "steps": a.steps, "opt": a.opt}
    for k, v in med.items():
        out[k] = {"step_ms": round(v * 1e3, 3), "emb_per_s": round(B / v, 1),
                  "spread_ms": [round(min(times[k]) * 1e3, 3), round(max(times[k]) * 1e3, 3)]}
    gf = campplus_gflop_per_utt(model.spec, T)
    out["gflop_per_utt"] = round(gf, 3)
    out["hip"]["tflops"] = round(gf * B / med["hip"] / 1e3, 2)
    out["hip_over_unfused"] = round(med["unfused"] / med["hip"], 3)
    model.set_option("cam_fused", 1)
    hip()
    if "eager" in med:
        out["hip_over_eager"] = round(med["eager"] / med["hip"], 3)
        out["max_abs_diff_vs_eager"] = float((emb - variants["eager"][1]()).abs().max())
    # per-class times, profiler on, in a run of its own (one stream: a launch is timed alone)
    model.set_option("streams", 1)
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
    assert torch.isfinite(emb).all()
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
