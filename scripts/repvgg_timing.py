"""RepVGG (feat 80 / embed 256) on one GPU: step time, embeddings per second, executed TF/s, the per-class
times of the handle's profiler and, for a RepSPK model, the 17-tap kernel against the dense 25-tap path
(option rsbb_taps: 2 = the 17 live taps wherever a block allows, 0 = all 25 taps on the 2-D implicit GEMM,
1 = the shipped per-stage choice) in interleaved pairs: whole model, and per stage from the kernel times.

    python scripts/repvgg_timing.py [--arch REPVGG_TINY_RSBB_A0] [--batch 64] [--frames 200] [--pairs 3]
                                    [--steps 5] [--eager] [--opt key=value ...]

Every variant is warmed up at the timed shape; a window is `steps` forwards between device synchronisations.
`pairs` lists, per pair, the window of rsbb_taps = 2 and right after it that of rsbb_taps = 0 (ms per step);
`stage_ms` the summed kernel time of each stage's blocks under either setting, from profiler runs of their
own (three each, alternating), with the MFMA floor of the 17-tap contraction (3 bf16 MFMA passes per MAC at
the dense bf16 peak) and the HBM floor (input + output activations once) beside it.  --eager adds
tests/repvgg_ref.py (torch functional ops, f32, deploy form) on the same GPU and shape.  Prints one JSON line
(development tool, not part of the bench contract)."""
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
import repvgg_ref  # noqa: E402
from repvgg_cases import tame  # noqa: E402
from wespeaker_hubert_amd import arch as A  # noqa: E402
from wespeaker_hubert_amd.speaker_model import HipSpeakerModel  # noqa: E402
from wespeaker_hubert_amd.synthetic import synth_feats, synth_state_dict  # noqa: E402

TAGS = ("stem", "rep_conv3x3", "rsbb_sparse", "rsbb_dense", "tstp_head")
PEAK_BF16_TFLOPS, PEAK_HBM_TBS = 2500.0, 8.0  # MI355X dense bf16 MFMA and HBM3E peaks


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--arch", default="REPVGG_TINY_RSBB_A0")
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--frames", type=int, default=200)
    ap.add_argument("--pairs", type=int, default=3)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--eager", action="store_true")
    ap.add_argument("--opt", action="append", default=[], help="handle option, e.g. streams=2")
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(0)
    B, T = a.batch, a.frames
    model = HipSpeakerModel(a.arch, feat_dim=80, embed_dim=256)
    spec = model.spec
    sd = tame(synth_state_dict(191, model.state_dict_layout()))
    model.load_state_dict(sd)
    for kv in a.opt:
        k, _, v = kv.partition("=")
        model.set_option(k, int(v))
    model.to(dev)
    spk = A.repvgg_kernel_size(spec) == 5
    feats = torch.from_numpy(synth_feats(7, B, T, 80)).to(dev)
    emb = torch.empty(B, 256, device=dev)

    def window(taps=None):
        if taps is not None:
            model.set_option("rsbb_taps", taps)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(a.steps):
            model.embed(feats, out=emb)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / a.steps

    keep = model.get_option("rsbb_taps")
    for taps in ((2, 0, keep) if spk else (None,)):  # warm up every variant at the timed shape
        window(taps)
    out = {"arch": a.arch, "batch": B, "frames": T, "pairs": a.pairs, "steps": a.steps, "opt": a.opt, "rsbb_taps": keep}
    shipped = [window(keep if spk else None) for _ in range(a.pairs)]
    med = statistics.median(shipped)
    gf = A.repvgg_gflop_per_utt(spec, T, 1 if keep else 0)
    out["hip"] = {"step_ms": round(med * 1e3, 3), "emb_per_s": round(B / med, 1),
                  "spread_ms": [round(min(shipped) * 1e3, 3), round(max(shipped) * 1e3, 3)],
                  "gflop_per_utt": round(gf, 3), "tflops": round(gf * B / med / 1e3, 2)}
    if a.eager:
        fsd = {k: torch.from_numpy(v).to(dev) for k, v in A.repvgg_fold(spec, sd).items()}
        with torch.no_grad():
            ref = repvgg_ref.forward(feats, fsd, a.arch)
            torch.cuda.synchronize()
            te = []
            for _ in range(a.pairs):
                t0 = time.perf_counter()
                for _ in range(a.steps):
                    repvgg_ref.forward(feats, fsd, a.arch)
                torch.cuda.synchronize()
                te.append((time.perf_counter() - t0) / a.steps)
        e = statistics.median(te)
        model.embed(feats, out=emb)
        out["eager"] = {"step_ms": round(e * 1e3, 3), "emb_per_s": round(B / e, 1)}
        out["hip_over_eager"] = round(e / med, 3)
        out["max_abs_diff_vs_eager"] = float((emb - ref).abs().max())

    def classes():
        torch.cuda.synchronize()
        model.profile(True)
        for _ in range(a.steps):
            model.embed(feats, out=emb)
        torch.cuda.synchronize()
        model.profile(False)
        return {t: model.profile_query(t) for t in TAGS + tuple(f"rsbb_{k}.L{li}" for k in ("sparse", "dense")
                                                                for li in (1, 2, 3, 4))}

    if spk:
        out["pairs_ms"] = [[round(window(2) * 1e3, 3), round(window(0) * 1e3, 3)] for _ in range(a.pairs)]
        out["sparse_over_dense_speedup"] = round(statistics.median(p[1] / p[0] for p in out["pairs_ms"]), 3)
        both = {}
        for v in (2, 0):
            model.set_option("rsbb_taps", v)
            both[v] = model.embed(feats).clone()
        out["max_abs_diff_sparse_vs_dense"] = float((both[2] - both[0]).abs().max())
        # per stage: kernel times under either setting, three alternating profiler runs each
        stage = {f"L{li}": {"sparse_ms": [], "dense_ms": []} for li in (1, 2, 3, 4)}
        for _ in range(a.pairs):
            for taps, kind in ((2, "sparse"), (0, "dense")):
                model.set_option("rsbb_taps", taps)
                q = classes()
                for li in (1, 2, 3, 4):
                    stage[f"L{li}"][kind + "_ms"].append(round(q[f"rsbb_{kind}.L{li}"][1] / a.steps, 4))
        # floors of a stage's 17-tap blocks: MACs x 3 MFMA passes at the bf16 peak; activations in + out once
        F, t = spec.feat_dim, T
        fl = {f"L{li}": [0.0, 0.0] for li in (1, 2, 3, 4)}
        for p, li, cin, cout, stride, _ in A.repvgg_blocks(spec):
            Fo, to = (F - 1) // stride + 1, (t - 1) // stride + 1
            if li:
                fl[f"L{li}"][0] += 3 * 2.0 * B * Fo * to * cout * cin * 17 / (PEAK_BF16_TFLOPS * 1e12) * 1e3
                fl[f"L{li}"][1] += 4.0 * B * (F * t * cin + Fo * to * cout) / (PEAK_HBM_TBS * 1e12) * 1e3
            F, t = Fo, to
        for k, v in stage.items():
            v["mfma_floor_ms"], v["hbm_floor_ms"] = round(fl[k][0], 4), round(fl[k][1], 4)
            v["sparse_wins_every_pair"] = all(s < d for s, d in zip(v["sparse_ms"], v["dense_ms"]))
        out["stage_ms"] = stage
        model.set_option("rsbb_taps", keep)
    q = classes()
    out["classes"] = {t: {"launches_per_step": q[t][0] // a.steps, "ms_per_step": round(q[t][1] / a.steps, 4),
                          "tflops": round(q[t][2] * q[t][0] / (q[t][1] * 1e-3) / 1e12, 2) if q[t][2] else None}
                      for t in TAGS if q[t][0]}
    assert torch.isfinite(emb).all()
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
