"""XVEC / XI_VEC_XVEC / XI_VEC_ECAPA_TDNN_* on one GPU: step time, embeddings per second, algorithmic
TF/s, the per-class times of the handle's profiler (xi_pool against its two-tensor HBM floor), ragged
batches against batch-of-one forwards, and the same model in eager torch for scale.

    python scripts/xvec_timing.py [--arch XVEC] [--batch 256] [--frames 200] [--repeats 5] [--steps 3]
                                  [--eager] [--ragged] [--opt key=value ...]

The HIP path is timed in `repeats` windows of `steps` forwards between device synchronisations and
reported as the median; --eager adds tests/xvec_ref.py (torch functional ops, f32) on the same GPU
and shape; --ragged times 64 utterances of 2 - 10 s (200 - 1000 frames) as one embed_segments call
against 64 batch-of-one forwards.  The per-class times come from a run of their own with the
profiler on.  Prints one JSON line (development tool, not part of the bench contract)."""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))
import xvec_ref  # noqa: E402
from wespeaker_hubert_amd.arch import ecapa_gflop_per_utt, xvec_gflop_per_utt  # noqa: E402
from wespeaker_hubert_amd.speaker_model import HipSpeakerModel  # noqa: E402
from wespeaker_hubert_amd.synthetic import synth_feats, synth_state_dict  # noqa: E402

TAGS = ("tdnn_k5", "tdnn_k3", "tdnn_1x1", "tstp", "layer1", "conv1x1_CxC", "res2_k3", "se", "se.scale", "conv_cat",
        "xi_lin1", "xi_lin2", "xi_pool", "head")
HBM_TBS = 6.3  # the achievable HBM rate the rooflines in DESIGN.md use


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
    ap.add_argument("--arch", default="XVEC")
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--frames", type=int, default=200)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--eager", action="store_true")
    ap.add_argument("--ragged", action="store_true")
    ap.add_argument("--opt", action="append", default=[], help="handle option, e.g. streams=2")
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(0)
    B, T = a.batch, a.frames
    ecapa = "ECAPA" in a.arch
    E = 192 if ecapa else 512
    model = HipSpeakerModel(a.arch, feat_dim=80, embed_dim=E)
    sd = synth_state_dict(83, model.state_dict_layout())
    model.load_state_dict(sd)
    for kv in a.opt:
        k, _, v = kv.partition("=")
        model.set_option(k, int(v))
    model.to(dev)
    feats = torch.from_numpy(synth_feats(7, B, T, 80)).to(dev)
    emb = torch.empty(B, E, device=dev)

    def hip():
        model.embed(feats, out=emb)

    med, lo, hi = _timed(hip, a.repeats, a.steps)
    gf = (ecapa_gflop_per_utt if ecapa else xvec_gflop_per_utt)(model.spec, T)
    out = {"arch": a.arch, "batch": B, "frames": T, "repeats": a.repeats, "steps": a.steps, "opt": a.opt,
           "gflop_per_utt": round(gf, 3),
           "hip": {"step_ms": round(med * 1e3, 3), "emb_per_s": round(B / med, 1), "tflops": round(gf * B / med / 1e3, 2),
                   "spread_ms": [round(lo * 1e3, 3), round(hi * 1e3, 3)]}}
    if a.eager:
        sd_dev = {k: torch.from_numpy(v).to(dev) for k, v in sd.items() if not k.endswith("num_batches_tracked")}
        eager = lambda: xvec_ref.forward(feats, sd_dev, a.arch, model.spec.pooling_func)  # noqa: E731
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
    classes = {}
    for t in TAGS:
        n, ms, fl = model.profile_query(t)
        if n:
            classes[t] = {"launches_per_step": n // a.steps, "ms_per_step": round(ms / a.steps, 4),
                          "tflops": round(fl * n / (ms * 1e-3) / 1e12, 2) if fl else None}
    if "xi_pool" in classes:
        # the kernel reads the logits and the activations once: 2 x rows x ld f32 (ld = 1536 on both families)
        rows = B * (T if ecapa else T - 14)
        floor_ms = 2 * rows * 1536 * 4 / (HBM_TBS * 1e12) * 1e3
        classes["xi_pool"]["hbm_floor_ms"] = round(floor_ms, 4)
        classes["xi_pool"]["of_floor"] = round(classes["xi_pool"]["ms_per_step"] / floor_ms, 2)
    out["classes"] = classes
    if a.ragged:
        rng = np.random.default_rng(5)
        lens = rng.integers(200, 1001, 64)
        utts = [torch.from_numpy(synth_feats(100 + i, 1, int(n), 80)).to(dev) for i, n in enumerate(lens)]
        packed = torch.cat([u[0] for u in utts])
        off = torch.tensor(np.concatenate([[0], np.cumsum(lens)]), dtype=torch.int32, device=dev)
        r_med, _, _ = _timed(lambda: model.embed_segments(packed, off), a.repeats, a.steps)
        o_med, _, _ = _timed(lambda: [model.embed(u) for u in utts], a.repeats, a.steps)
        out["ragged"] = {"utterances": 64, "frames": int(lens.sum()), "segments_ms": round(r_med * 1e3, 3),
                         "batch_of_one_ms": round(o_med * 1e3, 3), "speedup": round(o_med / r_med, 2)}
    assert torch.isfinite(emb).all()
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
