"""CAM++ (CAMPPlus) restated from its state_dict with torch functional ops on the CPU.

`forward(feats, sd, dtype)` computes what `CAMPPlus(feat_dim, embed_dim).eval()(feats)` computes
(FCM head, strided TDNN, three CAM dense-TDNN blocks with transits, TSTP, embedding) without the
module classes: every tensor comes from the state_dict by name.  `dtype=torch.float64` runs the
same graph in double precision.  `forward(..., taps=True)` also returns the intermediate tensors
the golden fixtures record (FCM output, xvector.tdnn, each block and transit, the frame-level
features in front of the pooling).
"""
import torch
import torch.nn.functional as F

LAYERS, DILATION, SEG = (12, 24, 16), (1, 2, 2), 100
EPS = 1e-5


def _bn(x, sd, p, affine=True):
    shape = [1, -1] + [1] * (x.dim() - 2)
    y = (x - sd[p + ".running_mean"].view(shape)) / torch.sqrt(sd[p + ".running_var"].view(shape) + EPS)
    if affine:
        y = y * sd[p + ".weight"].view(shape) + sd[p + ".bias"].view(shape)
    return y


def _res_block(x, sd, p, stride):
    out = F.relu(_bn(F.conv2d(x, sd[p + ".conv1.weight"], stride=(stride, 1), padding=1), sd, p + ".bn1"))
    out = _bn(F.conv2d(out, sd[p + ".conv2.weight"], padding=1), sd, p + ".bn2")
    if stride != 1:
        x = _bn(F.conv2d(x, sd[p + ".shortcut.0.weight"], stride=(stride, 1)), sd, p + ".shortcut.1")
    return F.relu(out + x)


def fcm(x, sd):
    """(B, F, T) -> (B, 32 * F / 8, T), channel c * F/8 + f."""
    out = F.relu(_bn(F.conv2d(x.unsqueeze(1), sd["head.conv1.weight"], padding=1), sd, "head.bn1"))
    for stage in (1, 2):
        out = _res_block(out, sd, f"head.layer{stage}.0", 2)
        out = _res_block(out, sd, f"head.layer{stage}.1", 1)
    out = F.relu(_bn(F.conv2d(out, sd["head.conv2.weight"], stride=(2, 1), padding=1), sd, "head.bn2"))
    return out.reshape(out.shape[0], out.shape[1] * out.shape[2], out.shape[3])


def segment_context(h):
    """mean over all frames + the mean of each frame's own 100-frame segment (the last segment
    averages its own frames only: avg_pool1d(ceil_mode=True))."""
    T = h.shape[-1]
    seg = torch.cat([h[..., s:s + SEG].mean(-1, keepdim=True).expand(-1, -1, min(SEG, T - s))
                     for s in range(0, T, SEG)], dim=-1)
    return h.mean(-1, keepdim=True) + seg


def dense_layer(x, sd, p, dil):
    h = F.conv1d(F.relu(_bn(x, sd, p + ".nonlinear1.batchnorm")), sd[p + ".linear1.weight"])
    h = F.relu(_bn(h, sd, p + ".nonlinear2.batchnorm"))
    c = p + ".cam_layer"
    y = F.conv1d(h, sd[c + ".linear_local.weight"], padding=dil, dilation=dil)
    ctx = F.relu(F.conv1d(segment_context(h), sd[c + ".linear1.weight"], sd[c + ".linear1.bias"]))
    m = torch.sigmoid(F.conv1d(ctx, sd[c + ".linear2.weight"], sd[c + ".linear2.bias"]))
    return y * m


def forward(feats, sd, dtype=torch.float32, taps=False):
    """feats (B, T, F) -> embedding (B, embed_dim); with taps also a dict of intermediates."""
    sd = {k: torch.as_tensor(v).to(dtype) for k, v in sd.items() if not k.endswith("num_batches_tracked")}
    inter = {}
    with torch.no_grad():
        x = fcm(torch.as_tensor(feats).to(dtype).permute(0, 2, 1), sd)
        inter["head"] = x
        x = F.conv1d(x, sd["xvector.tdnn.linear.weight"], stride=2, padding=2)
        x = F.relu(_bn(x, sd, "xvector.tdnn.nonlinear.batchnorm"))
        inter["tdnn"] = x
        for b, (n, dil) in enumerate(zip(LAYERS, DILATION)):
            for i in range(n):
                x = torch.cat([x, dense_layer(x, sd, f"xvector.block{b + 1}.tdnnd{i + 1}", dil)], dim=1)
            inter[f"block{b + 1}"] = x
            t = f"xvector.transit{b + 1}"
            x = F.conv1d(F.relu(_bn(x, sd, t + ".nonlinear.batchnorm")), sd[t + ".linear.weight"])
            inter[f"transit{b + 1}"] = x
        x = F.relu(_bn(x, sd, "xvector.out_nonlinear.batchnorm"))
        inter["frame_level"] = x.permute(0, 2, 1)
        stats = torch.cat([x.mean(-1), torch.sqrt(x.var(-1, unbiased=True) + 1e-7)], dim=-1)
        e = F.conv1d(stats.unsqueeze(-1), sd["xvector.dense.linear.weight"]).squeeze(-1)
        e = _bn(e, sd, "xvector.dense.nonlinear.batchnorm", affine=False)
    return (e, inter) if taps else e
