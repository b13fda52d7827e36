"""Res2Net (Res2Net34_Base / _Large) restated on torch-CPU from the model's description: the project's
own oracle for the HIP path.  Eval-mode BatchNorms are applied as they are (no folding), in the
dtype asked for.

    forward(x, sd, arch, ...) -> embedding [B][embed_dim]  (and the named intermediates with taps=True)

x: (B, T, feat_dim) features, sd: state dict keyed by the reference names (numpy or torch, on any one
device).  A block with width w = planes / 2:
    y   = clamp(bn1(conv1_1x1,stride(x)))                 2w channels
    s   = clamp(bns.0(convs.0_3x3(y[:, :w])))
    out = clamp(bn3(conv3_1x1([s | y[:, w:]])) + shortcut(x))
clamp=False replaces every clamp(., 0, 20) by a plain ReLU (the tests use it to show that an input
exercises the ceiling).  macs=True also returns the multiply-accumulates of every conv / linear of one
utterance, counted from the shapes of the calls made here.
"""
import torch
import torch.nn.functional as F

from wespeaker_hubert_amd import arch as A

TAPS = ("stem", "layer1", "layer2", "layer3", "layer4")


def forward(x, sd, arch="Res2Net34_Base", two_emb_layer=False, clamp=True, dtype=torch.float32, taps=False,
            macs=False):
    sd = {k: torch.as_tensor(v).to(dtype) for k, v in sd.items()}
    x = torch.as_tensor(x).to(dtype)
    spec = A.make_spec(arch, feat_dim=x.shape[2], embed_dim=sd["seg_1.weight"].shape[0], two_emb_layer=two_emb_layer)
    count = [0]

    def conv(v, name, **kw):
        w = sd[name + ".weight"]
        o = F.conv2d(v, w, **kw)
        count[0] += o.shape[2] * o.shape[3] * w.numel()  # per utterance
        return o

    def linear(v, name):
        count[0] += sd[name + ".weight"].numel()
        return F.linear(v, sd[name + ".weight"], sd[name + ".bias"])

    def bn(p, v):
        return F.batch_norm(v, sd[p + ".running_mean"], sd[p + ".running_var"], sd[p + ".weight"], sd[p + ".bias"],
                            False, 0.0, 1e-5)

    def act(v):
        return v.clamp(0.0, 20.0) if clamp else v.clamp_min(0.0)

    inter = {}
    out = F.relu(bn("bn1", conv(x.transpose(1, 2).unsqueeze(1), "conv1", padding=1)))
    inter["stem"] = out
    for p, _, _, w, stride, has_sc in A.res2net_blocks(spec):
        y = act(bn(p + ".bn1", conv(out, p + ".conv1", stride=stride)))
        s = act(bn(p + ".bns.0", conv(y[:, :w], p + ".convs.0", padding=1)))
        z = bn(p + ".bn3", conv(torch.cat((s, y[:, w:]), 1), p + ".conv3"))
        res = out
        if has_sc:
            res = bn(p + ".shortcut.1", conv(out, p + ".shortcut.0", stride=stride))
        out = act(z + res)
        inter[p.split(".")[0]] = out  # the stage's last block stays
    # TSTP over (B, C, F, T) flattened channel-major (C, F): mean | unbiased std
    v = out.reshape(out.shape[0], -1, out.shape[3])
    stats = torch.cat((v.mean(-1), torch.sqrt(v.var(-1, unbiased=True) + 1e-7)), 1)
    emb = linear(stats, "seg_1")
    if two_emb_layer:
        r = F.relu(emb)
        r = (r - sd["seg_bn_1.running_mean"]) / torch.sqrt(sd["seg_bn_1.running_var"] + 1e-5)
        emb = linear(r, "seg_2")
    ret = (emb,) + ((inter,) if taps else ()) + ((count[0],) if macs else ())
    return ret if len(ret) > 1 else emb
