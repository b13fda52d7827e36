"""The x-vector TDNN, the XI pooling layer and the XI-ECAPA tail restated on torch-CPU from the
models' description: the project's own oracle for the HIP path, in the dtype asked for (float64 is
the oracle).  Eval-mode BatchNorms are applied as they are (no folding).

    forward(x, sd, arch, pooling_func=None, emb_bn=False) -> embedding [B][embed_dim]

x: (B, T, feat_dim) features, sd: state dict keyed by the reference names.  For XVEC the result is
embed_b (the reference's outputs[-1]).  The ECAPA trunk is oracle/models_ref.py's.
"""
import torch
import torch.nn.functional as F

from oracle import models_ref
from wespeaker_hubert_amd import arch as A

TAPS = ("frame_1", "frame_3", "frame_5", "pool")


def _bn(v, sd, p):
    """Eval BatchNorm over dim 1, with or without affine."""
    shape = [1, -1] + [1] * (v.dim() - 2)
    y = (v - sd[p + ".running_mean"].view(shape)) / torch.sqrt(sd[p + ".running_var"].view(shape) + 1e-5)
    if p + ".weight" in sd:
        y = y * sd[p + ".weight"].view(shape) + sd[p + ".bias"].view(shape)
    return y


def xi_logits(x, sd, p="pool"):
    """z = lin2(BN(ReLU(lin1(x)))) for x (B, D, T)."""
    h = F.relu(F.conv1d(x, sd[p + ".lin1_relu_bn.0.weight"], sd[p + ".lin1_relu_bn.0.bias"]))
    return F.conv1d(_bn(h, sd, p + ".lin1_relu_bn.2"), sd[p + ".lin2.weight"], sd[p + ".lin2.bias"])


def xi_closed_form(z, x, prior_mean, prior_logprec):
    """phi = (sum_t s_t^2 x_t + e^lp m) / (sum_t s_t^2 + e^lp), s = softplus(z) (threshold 20)."""
    s2 = F.softplus(z, beta=1, threshold=20) ** 2
    w0 = torch.exp(prior_logprec)  # (1, D)
    return ((s2 * x).sum(2) + w0 * prior_mean) / (s2.sum(2) + w0)


def xi_softmax_form(z, x, prior_mean, prior_logprec):
    """The layer as it is described: softmax over the T log-precisions 2 log softplus(z) plus the
    prior's, applied to [x_t ..., prior_mean]."""
    B = z.shape[0]
    lp = torch.cat((2.0 * torch.log(F.softplus(z, beta=1, threshold=20)), prior_logprec.repeat(B, 1).unsqueeze(2)), 2)
    v = torch.cat((x, prior_mean.repeat(B, 1).unsqueeze(2)), 2)
    return (v * torch.softmax(lp, dim=2)).sum(2)


def xi_pool(x, sd, p="pool"):
    return xi_closed_form(xi_logits(x, sd, p), x, sd[p + ".prior_mean"], sd[p + ".prior_logprec"])


def xvec_forward(x, sd, pooling_func, taps=False):
    out = x.transpose(1, 2)  # (B, T, F) -> (B, F, T)
    inter = {}
    for i, (_, dil) in enumerate(A.XVEC_FRAMES, 1):
        p = f"frame_{i}"
        out = _bn(F.relu(F.conv1d(out, sd[p + ".conv_1d.weight"], sd[p + ".conv_1d.bias"], dilation=dil)), sd, p + ".bn")
        inter[p] = out
    if pooling_func == "XI":
        stats = xi_pool(out, sd)
    else:
        stats = torch.cat((out.mean(-1), torch.sqrt(out.var(-1, unbiased=True) + 1e-7)), 1)
    inter["pool"] = stats
    r = _bn(F.relu(F.linear(stats, sd["seg_1.weight"], sd["seg_1.bias"])), sd, "seg_bn_1")
    emb = F.linear(r, sd["seg_2.weight"], sd["seg_2.bias"])
    return (emb, inter) if taps else emb


def xi_ecapa_forward(x, sd, emb_bn=False, taps=False):
    out, _, _ = models_ref.ecapa_frame_level(x, sd)
    pooled = xi_pool(F.relu(out), sd)
    e = F.linear(_bn(pooled, sd, "bn"), sd["linear.weight"], sd["linear.bias"])
    if emb_bn:
        e = _bn(e, sd, "bn2")
    return (e, {"pool": pooled}) if taps else e


def forward(x, sd, arch, pooling_func=None, emb_bn=False, dtype=torch.float32, taps=False):
    sd = {k: torch.as_tensor(v).to(dtype) for k, v in sd.items() if not k.endswith("num_batches_tracked")}
    x = torch.as_tensor(x).to(dtype)
    with torch.no_grad():
        if arch in A.XI_ECAPA_ARCHS:
            return xi_ecapa_forward(x, sd, emb_bn, taps)
        return xvec_forward(x, sd, pooling_func or A.XVEC_ARCHS[arch], taps)
