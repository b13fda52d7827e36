"""Pins tests/wavlm_ref.py (WavLM Base / Base+ restatement) against the transformers
WavLMModel proxy fixture (tests/golden/wavlm_proxy.npz, made by
tests/golden/make_wavlm_proxy.py) at test_hubert_oracle.py's tolerances (|Δ| ≤ 2e-4
per element on LayerNorm-scaled O(1) states, rtol 1e-5 on abs-sums), and checks the
relative-position bucket rule and the S3prlFrontend constructor's upstream names."""
import math
import os

import numpy as np
import pytest
import torch

from wavlm_ref import rel_bucket, rel_buckets, s3prl_frontend, wavlm_hidden_states
from wespeaker_hubert_amd.arch import (HUBERT_PREFIX, hubert_params, s3prl_num_frames, wavlm_params,
                                       wavlm_rel_bucket)
from wespeaker_hubert_amd.synthetic import synth_audio, synth_state_dict

GOLD = os.path.join(os.path.dirname(__file__), "golden", "wavlm_proxy.npz")


@pytest.fixture(scope="module")
def gold():
    return np.load(GOLD)


@pytest.fixture(scope="module")
def sd(gold):
    raw = synth_state_dict(int(gold["weight_seed"]), wavlm_params())
    return {k: torch.from_numpy(v) for k, v in raw.items()}


def test_param_layout():
    hub = hubert_params()
    wav = wavlm_params()
    names = [n for n, _ in wav]
    assert len(names) == len(set(names))
    extra = [(n, s) for n, s in wav if (n, s) not in hub]
    assert [x for x in wav if x in hub] == hub  # HuBERT's entries, in HuBERT's order
    assert len(extra) == 12 * 3 + 1
    pre = HUBERT_PREFIX + "encoder.layers."
    assert (pre + "0.self_attn.relative_attention_bias.weight", (320, 12)) in extra
    for li in range(12):
        assert (pre + f"{li}.self_attn.grep_linear.weight", (8, 64)) in extra
        assert (pre + f"{li}.self_attn.grep_linear.bias", (8,)) in extra
        assert (pre + f"{li}.self_attn.grep_a", (1, 12, 1, 1)) in extra
    assert dict(wav)["frontend.featurizer.weights"] == (13,)
    # HF WavLMModel(WavLMConfig()) minus masked_spec_embed, + featurizer
    assert sum(int(np.prod(s)) for _, s in wav) == 94371712 - 768 + 13 + 320 * 12 + 12 * (8 * 64 + 8 + 12)


def _rule(d):
    """The bucket rule, written out independently: n = 160; bucket = (d > 0) * n; r = |d|;
    r < 80 adds r, otherwise min(159, int(80 + log(r / 80) / log(800 / 80) * 80))."""
    b = 160 if d > 0 else 0
    r = -d if d < 0 else d
    if r < 80:
        return b + r
    return b + min(159, int(80 + math.log(r / 80) / math.log(800 / 80) * 80))


def test_bucket_rule():
    T = 1201
    tab = rel_buckets(T)  # fp32 tensor arithmetic, as the model computes it
    for d in range(-1200, 1201):
        want = _rule(d)
        assert rel_bucket(d) == want and wavlm_rel_bucket(d) == want, d
        i, j = (0, d) if d >= 0 else (-d, 0)  # query i, key j, d = j - i
        assert int(tab[i, j]) == want, d
    assert tab.min() == 0 and tab.max() == 319


def test_bucket_saturation_and_sign():
    # constant from |d| = 778 on: one table over [-778, 778] with clamping is exact
    assert rel_bucket(777) == 318 and rel_bucket(-777) == 158
    assert all(rel_bucket(d) == 319 for d in range(778, 1201))
    assert all(rel_bucket(-d) == 159 for d in range(778, 1201))
    # d > 0: the key comes after the query and takes the upper 160
    assert rel_bucket(0) == 0 and rel_bucket(1) == 161 and rel_bucket(-1) == 1
    assert rel_bucket(79) == 239 and rel_bucket(-79) == 79 and rel_bucket(80) == 240 and rel_bucket(-80) == 80
    tab = rel_buckets(4)
    assert int(tab[0, 3]) == 163 and int(tab[3, 0]) == 3  # [query][key]


@pytest.mark.parametrize("tag", ["short", "long"])
def test_hidden_states_vs_proxy(gold, sd, tag):
    wav = torch.from_numpy(synth_audio(int(gold[f"{tag}_wav_seed"]), int(gold[f"{tag}_batch"]),
                                       int(gold[f"{tag}_num_samples"]), int16_scale=False))
    with torch.no_grad():
        hs = wavlm_hidden_states(wav, sd)
    assert len(hs) == 13
    sums = np.array([h.double().sum().item() for h in hs])
    abss = np.array([h.double().abs().sum().item() for h in hs])
    np.testing.assert_allclose(abss, gold[f"{tag}_layer_abs"], rtol=1e-5)
    np.testing.assert_allclose(sums, gold[f"{tag}_layer_sums"], atol=1e-5 * abss.max())
    if tag == "short":
        np.testing.assert_allclose(hs[0][:1].numpy(), gold["short_hs0"], atol=2e-4, rtol=0)
        for i in (1, 12):
            np.testing.assert_allclose(hs[i].numpy(), gold[f"short_hs{i}"], atol=2e-4, rtol=0)
    else:
        assert hs[1].shape[1] > 80  # the log-spaced buckets are in play
        for i in (1, 12):
            ends = np.concatenate([hs[i][0, :8].numpy(), hs[i][0, -8:].numpy()])
            np.testing.assert_allclose(ends, gold[f"long_hs{i}"], atol=2e-4, rtol=0)


def test_bias_matters(gold, sd):
    """The fixture discriminates: without the bias table hidden state 1 moves by far more than 2e-4."""
    wav = torch.from_numpy(synth_audio(int(gold["short_wav_seed"]), 2, 8000, int16_scale=False))
    k = HUBERT_PREFIX + "encoder.layers.0.self_attn.relative_attention_bias.weight"
    with torch.no_grad():
        hs = wavlm_hidden_states(wav, dict(sd, **{k: torch.zeros_like(sd[k])}))
    assert np.abs(hs[1].numpy() - gold["short_hs1"]).max() > 0.02


def test_featurizer_glue(sd):
    wav = torch.from_numpy(synth_audio(3, 1, 4000, int16_scale=False))
    with torch.no_grad():
        f = s3prl_frontend(wav, sd)
        short = s3prl_frontend(wav[:, :600], sd)
        pad = s3prl_frontend(torch.nn.functional.pad(wav[:, :600], (0, 200)), sd)
    assert f.shape == (1, s3prl_num_frames(4000), 768) and torch.isfinite(f).all()
    assert short.shape == (1, 2, 768)  # MIN_SECOND: run zero-padded to 800 samples, 2 frames kept
    torch.testing.assert_close(short, pad[:, :2], rtol=0, atol=0)


# ------------------------------------------------ S3prlFrontend construction ---
def test_frontend_accepts_wavlm_names():
    from wespeaker_hubert_amd.s3prl_frontend import S3prlFrontend
    for name in ("wavlm_base", "wavlm_base_plus"):
        fe = S3prlFrontend({"name": name})
        assert fe.output_size() == 768
        assert fe._create_args()[:3] == ("WavLM_base", 1, 768)
        assert fe._layout == wavlm_params()
    hub = S3prlFrontend({"name": "hubert_base"})
    assert hub._create_args()[:3] == ("HuBERT_base", 1, 768) and hub._layout == hubert_params()


def test_frontend_rejects_unsupported():
    from wespeaker_hubert_amd.s3prl_frontend import S3prlFrontend
    with pytest.raises(NotImplementedError, match="wavlm_large.*24 pre-LN"):
        S3prlFrontend({"name": "wavlm_large"})
    for name in ("wavlm", "wav2vec2", None):
        with pytest.raises(NotImplementedError, match="wavlm_base_plus"):  # the message names what is supported
            S3prlFrontend({"name": name})
    with pytest.raises(NotImplementedError, match="normalize"):
        S3prlFrontend({"name": "wavlm_base_plus", "normalize": True})
