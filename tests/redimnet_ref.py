"""ReDimNetB2 restated as plain torch functions over a state dict (no reference import): the checker
of the HIP path and of the fixtures' float64 embeddings.  Written from the module's structure
(redimnet.py:622-871, pooling_layers.py:92-144); `forward(x, sd, dtype=...)` runs it in float64 or
float32, `taps` collects the float64 sum / abs-sum of the stem and of every stage's 1-D output.

Layout facts the HIP path relies on, stated here once:
  to1d      (B, C, F, T) -> (B, F*C, T), 1-D channel f*C + c
  to2d      its inverse with the stage's (c, F)
  weigth1d  softmax over the *inputs* axis of inputs_weights[i] (1, i+1, 1152, 1), per channel
"""
from __future__ import annotations

import math

import numpy as np
import torch
import torch.nn.functional as F

from wespeaker_hubert_amd.arch import REDIMNET_ARCHS, REDIMNET_DW_KERNELS, REDIMNET_HEADS, redimnet_stage_dims

LN_EPS = 1e-6


def ln_cf(x, w, b):
    """channels-first LayerNorm over dim 1 (biased variance, eps 1e-6)"""
    u = x.mean(1, keepdim=True)
    s = (x - u).pow(2).mean(1, keepdim=True)
    x = (x - u) / torch.sqrt(s + LN_EPS)
    shape = (1, -1) + (1,) * (x.dim() - 2)
    return w.view(shape) * x + b.view(shape)


def new_gelu(x):
    return 0.5 * x * (1.0 + torch.tanh(math.sqrt(2.0 / math.pi) * (x + 0.044715 * x.pow(3))))


def _bn(x, sd, p):
    shape = (1, -1) + (1,) * (x.dim() - 2)
    sc = sd[p + ".weight"] / torch.sqrt(sd[p + ".running_var"] + 1e-5)
    return (x - sd[p + ".running_mean"].view(shape)) * sc.view(shape) + sd[p + ".bias"].view(shape)


def convnext2d(x, sd, p, groups):
    y = F.conv2d(x, sd[p + ".dwconvs.0.weight"], sd[p + ".dwconvs.0.bias"], padding=1, groups=groups)
    y = F.gelu(_bn(y, sd, p + ".norm"))
    return x + F.conv2d(y, sd[p + ".pwconv1.weight"], sd[p + ".pwconv1.bias"])


def convnext1d(x, sd, p):
    w = sd[p + ".dwconvs.0.weight"]
    y = F.conv1d(x, w, sd[p + ".dwconvs.0.bias"], padding=w.shape[-1] // 2, groups=w.shape[0])
    y = F.gelu(_bn(y, sd, p + ".norm"))
    return x + F.conv1d(y, sd[p + ".pwconv1.weight"], sd[p + ".pwconv1.bias"])


def attention(h, sd, p, heads=REDIMNET_HEADS):
    """h (B, T, D): q scaled by dh^-0.5 after its bias, no mask, no position term"""
    B, T, D = h.shape
    dh = D // heads
    q = F.linear(h, sd[p + ".q_proj.weight"], sd[p + ".q_proj.bias"]) * dh ** -0.5
    k = F.linear(h, sd[p + ".k_proj.weight"], sd[p + ".k_proj.bias"])
    v = F.linear(h, sd[p + ".v_proj.weight"], sd[p + ".v_proj.bias"])
    q, k, v = (t.view(B, T, heads, dh).transpose(1, 2) for t in (q, k, v))
    a = torch.softmax(q @ k.transpose(-1, -2), dim=-1) @ v
    a = a.transpose(1, 2).reshape(B, T, D)
    return F.linear(a, sd[p + ".out_proj.weight"], sd[p + ".out_proj.bias"])


def transformer(x, sd, p):
    """post-LN encoder layer on (B, hC, T)"""
    h = x.transpose(1, 2)
    D = h.shape[-1]
    h = F.layer_norm(h + attention(h, sd, p + ".attention"), (D,), sd[p + ".layer_norm.weight"],
                     sd[p + ".layer_norm.bias"], LN_EPS)
    f = F.linear(h, sd[p + ".feed_forward.intermediate_dense.weight"], sd[p + ".feed_forward.intermediate_dense.bias"])
    f = F.linear(new_gelu(f), sd[p + ".feed_forward.output_dense.weight"], sd[p + ".feed_forward.output_dense.bias"])
    h = F.layer_norm(h + f, (D,), sd[p + ".final_layer_norm.weight"], sd[p + ".final_layer_norm.bias"], LN_EPS)
    return h.transpose(1, 2)


def block1d(x, sd, p):
    h = F.conv1d(x, sd[p + ".red_dim_conv.0.weight"], sd[p + ".red_dim_conv.0.bias"])
    h = ln_cf(h, sd[p + ".red_dim_conv.1.weight"], sd[p + ".red_dim_conv.1.bias"])
    for j in range(len(REDIMNET_DW_KERNELS)):
        h = convnext1d(h, sd, f"{p}.tcm.{j}")
    h = transformer(h, sd, p + ".tcm.4")
    return x + F.conv1d(h, sd[p + ".exp_dim_conv.weight"], sd[p + ".exp_dim_conv.bias"])


def weigth1d(outs, w):
    return (torch.softmax(w, dim=1) * torch.stack(outs, dim=1)).sum(dim=1)


def astp(x, sd):
    mean = x.mean(-1, keepdim=True).expand_as(x)
    std = torch.sqrt(x.var(-1, keepdim=True) + 1e-7).expand_as(x)
    a = torch.tanh(F.conv1d(torch.cat((x, mean, std), 1), sd["pool.linear1.weight"], sd["pool.linear1.bias"]))
    a = torch.softmax(F.conv1d(a, sd["pool.linear2.weight"], sd["pool.linear2.bias"]), dim=2)
    m = (a * x).sum(2)
    var = (a * x * x).sum(2) - m * m
    return torch.cat([m, torch.sqrt(var.clamp(min=1e-7))], 1)


def forward(x, sd, arch="ReDimNetB2", dtype=torch.float64, taps=None):
    """x (B, T, 72) array or tensor, sd a name -> array / tensor dict; returns the embedding (B, E)
    (embed_b with seg_2 in the state dict)."""
    as_t = lambda v: (v if torch.is_tensor(v) else torch.from_numpy(np.asarray(v))).to(dtype)  # noqa: E731  (keeps the device)
    sd = {k: as_t(v) for k, v in sd.items() if "num_batches" not in k}
    x = as_t(x)
    _, gd, _ = REDIMNET_ARCHS[arch]

    def tap(tag, t):
        if taps is not None:
            taps["sum_" + tag] = float(t.double().sum())
            taps["abs_" + tag] = float(t.double().abs().sum())

    with torch.no_grad():
        B, T, _ = x.shape
        h = F.conv2d(x.transpose(1, 2).unsqueeze(1), sd["backbone.stem.0.weight"], sd["backbone.stem.0.bias"], padding=1)
        h = ln_cf(h, sd["backbone.stem.1.weight"], sd["backbone.stem.1.bias"])
        tap("stem", h)
        outs = [h.permute(0, 2, 1, 3).reshape(B, -1, T)]
        for si, (ci, Fi, s, c, _, n, _) in enumerate(redimnet_stage_dims(arch)):
            p = f"backbone.stage{si}"
            h = weigth1d(outs, sd[f"backbone.inputs_weights.{si}"])
            h = h.reshape(B, Fi, ci, T).permute(0, 2, 1, 3)
            h = F.conv2d(h, sd[p + ".0.weight"], sd[p + ".0.bias"], stride=(s, 1))
            for bi in range(1, n + 1):
                h = convnext2d(h, sd, f"{p}.{bi}.conv_block", c // gd)
            h = block1d(h.permute(0, 2, 1, 3).reshape(B, -1, T), sd, f"{p}.{n + 2}")
            tap(f"stage{si}", h)
            outs.append(h)
        h = weigth1d(outs, sd[f"backbone.inputs_weights.{len(outs) - 1}"])
        e = F.linear(astp(h, sd), sd["seg_1.weight"], sd["seg_1.bias"])
        if "seg_2.weight" in sd:
            r = (F.relu(e) - sd["seg_bn_1.running_mean"]) / torch.sqrt(sd["seg_bn_1.running_var"] + 1e-5)
            e = F.linear(r, sd["seg_2.weight"], sd["seg_2.bias"])
    return e
