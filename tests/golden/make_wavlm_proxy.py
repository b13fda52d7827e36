"""Golden fixture for the WavLM Base / Base+ front end from transformers' WavLMModel
(offline third-party PROXY for s3prl's `wavlm_base` / `wavlm_base_plus`; s3prl is
absent and its weights download by URL, so reference parity is unpinned — DESIGN.md §3).

Synthetic weights are generated under the canonical names
(wespeaker_hubert_amd.arch.wavlm_params), mapped onto the transformers module, and the
13 hidden states are recorded: per-layer sums and abs-sums, plus a few states.  The
"long" input has 124 frames, so the log-spaced buckets (|d| >= 80) are in the fixture.
Run: python tests/golden/make_wavlm_proxy.py
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
sys.path.insert(0, HERE)

from make_hubert_proxy import fairseq_to_hf  # noqa: E402
from wespeaker_hubert_amd.arch import HUBERT_PREFIX, wavlm_params  # noqa: E402
from wespeaker_hubert_amd.synthetic import synth_audio, synth_state_dict  # noqa: E402

P = HUBERT_PREFIX
INPUTS = (("short", 61, 2, 8000), ("long", 62, 1, 40000))  # tag, audio seed, batch, samples (24 / 124 frames)


def wavlm_to_hf(name: str) -> str:
    n = fairseq_to_hf(name)
    n = n.replace(".attention.relative_attention_bias.", ".attention.rel_attn_embed.")
    n = n.replace(".attention.grep_linear.", ".attention.gru_rel_pos_linear.")
    n = n.replace(".attention.grep_a", ".attention.gru_rel_pos_const")
    return n


def main():
    from transformers import WavLMConfig, WavLMModel
    torch.manual_seed(0)
    model = WavLMModel(WavLMConfig()).eval()
    plist = [(n, s) for n, s in wavlm_params() if n.startswith(P)]
    sd = synth_state_dict(41, plist)
    hf = model.state_dict()
    new = {}
    for n, v in sd.items():
        k = wavlm_to_hf(n)
        assert k in hf, k
        assert tuple(hf[k].shape) == tuple(v.shape), (k, hf[k].shape, v.shape)
        new[k] = torch.from_numpy(v)
    missing = [k for k in hf if k not in new]
    assert missing == ["masked_spec_embed"], missing
    new["masked_spec_embed"] = hf["masked_spec_embed"]
    model.load_state_dict(new, strict=True)
    rec = {}
    for tag, seed, batch, n in INPUTS:
        wav = synth_audio(seed, batch, n, int16_scale=False)
        with torch.no_grad():
            out = model(torch.from_numpy(wav), output_hidden_states=True)
        hs = out.hidden_states
        assert len(hs) == 13
        rec[f"{tag}_wav_seed"] = np.int64(seed)
        rec[f"{tag}_batch"] = np.int64(batch)
        rec[f"{tag}_num_samples"] = np.int64(n)
        rec[f"{tag}_layer_sums"] = np.array([h.double().sum().item() for h in hs])
        rec[f"{tag}_layer_abs"] = np.array([h.double().abs().sum().item() for h in hs])
        if tag == "short":
            rec["short_hs0"] = hs[0][:1].numpy()  # before any attention: one utterance is enough
            for i in (1, 12):
                rec[f"short_hs{i}"] = hs[i].numpy()
        else:  # the rows at both ends: their far keys sit in the log-spaced buckets
            rec["long_hs1"] = np.concatenate([hs[1][0, :8].numpy(), hs[1][0, -8:].numpy()])
            rec["long_hs12"] = np.concatenate([hs[12][0, :8].numpy(), hs[12][0, -8:].numpy()])
        print(tag, hs[12].shape, float(hs[12].abs().max()))
    rec["weight_seed"] = np.int64(41)
    np.savez_compressed(os.path.join(HERE, "wavlm_proxy.npz"), **rec)


if __name__ == "__main__":
    main()
