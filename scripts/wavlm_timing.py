"""WavLM Base(+) front end + ECAPA_TDNN_GLOB_c512(768) at the C4 shape (B = 256 x 5 s, default
options): step time and embeddings / s, then the per-kernel-class times on ONE stream (as
scripts/class_times.py does for the bench workloads: with the default two utterance-range
streams a launch shares the GPU with the other range's kernels).

    python scripts/wavlm_timing.py [--batch 256] [--seconds 5] [--steps 5] [--upstream wavlm_base_plus]
                                   [--opt key=value ...]

`--upstream hubert_base` runs the same script on the HuBERT front end, for a like-for-like h_attn.
Prints one JSON line (development tool, not part of the bench contract)."""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
from wespeaker_hubert_amd.s3prl_frontend import S3prlFrontend  # noqa: E402
from wespeaker_hubert_amd.speaker_model import HipSpeakerModel  # noqa: E402
from wespeaker_hubert_amd.synthetic import synth_audio, synth_state_dict  # noqa: E402

FE_TAGS = ("h_conv0", "h_cnn", "h_ln", "h_proj", "h_pos_conv", "h_qkv", "h_gate", "h_attn", "h_out_proj", "h_fc1",
           "h_fc2", "h_cmn")


def class_times(handle, step, tags, steps):
    old = handle.get_option("streams")
    handle.set_option("streams", 1)
    try:
        step()
        torch.cuda.synchronize()
        handle.profile(True)
        for _ in range(steps):
            step()
        torch.cuda.synchronize()
        handle.profile(False)
        out = {}
        for t in tags:
            n, ms, _ = handle.profile_query(t)
            if n:
                out[t] = {"launches_per_step": n // steps, "avg_ms": round(ms / n, 4), "ms_per_step": round(ms / steps, 4)}
        return out
    finally:
        handle.set_option("streams", old)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--seconds", type=float, default=5.0)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--upstream", default="wavlm_base_plus")
    ap.add_argument("--opt", action="append", default=[])
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(0)
    B, N = a.batch, int(round(a.seconds * 16000))
    model = HipSpeakerModel("ECAPA_TDNN_GLOB_c512", feat_dim=768, embed_dim=192)
    model.load_state_dict(synth_state_dict(1234, model.state_dict_layout()))
    fe = S3prlFrontend({"name": a.upstream})
    fe.load_state_dict(synth_state_dict(1235, fe.state_dict_layout()))
    for kv in a.opt:
        k, _, v = kv.partition("=")
        fe.set_option(k, int(v))
    model.to(dev)
    fe.to(dev)
    wav = torch.from_numpy(synth_audio(7, B, N, int16_scale=False)).to(dev)
    feats = torch.empty(B, (N + 319) // 320, 768, device=dev)
    emb = torch.empty(B, 192, device=dev)

    def step():
        fe.extract(wav, cmn=True, out=feats)
        model.embed(feats, out=emb)

    for _ in range(a.warmup):
        step()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(a.steps):
        step()
    torch.cuda.synchronize()
    dt = (time.perf_counter() - t0) / a.steps
    assert torch.isfinite(emb).all()
    classes = class_times(fe, step, FE_TAGS, max(2, a.steps // 2))
    print(json.dumps({"upstream": a.upstream, "batch": B, "seconds": a.seconds, "step_ms": round(dt * 1e3, 3),
                      "emb_per_s": round(B / dt, 1), "classes_one_stream": classes}), flush=True)


if __name__ == "__main__":
    main()
