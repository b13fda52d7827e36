"""ERes2Net restated on torch-CPU from the model's description: the project's own oracle for the
HIP path.  Eval-mode BatchNorms are applied as they are (no folding), in the dtype asked for.

    forward(x, sd, arch, ...) -> embedding [B][embed_dim]  (and the named intermediates with taps=True)

x: (B, T, feat_dim) features, sd: state dict keyed by the reference names (numpy or torch, on
any one device).
clamp=False replaces every clamp(., 0, 20) by a plain ReLU: what the network would compute
without its Hardtanh ceiling (the tests use it to show that an input exercises the ceiling).
"""
import torch
import torch.nn.functional as F

from wespeaker_hubert_amd import arch as A

TAPS = ("stem", "layer1", "layer2", "layer3", "layer4", "down1", "fuse12", "down2", "fuse123", "down3", "fuse1234")


def forward(x, sd, arch="ERes2Net34_Base", two_emb_layer=False, clamp=True, dtype=torch.float32, taps=False):
    sd = {k: torch.as_tensor(v).to(dtype) for k, v in sd.items()}
    x = torch.as_tensor(x).to(dtype)
    spec = A.make_spec(arch, feat_dim=x.shape[2], embed_dim=sd["seg_1.weight"].shape[0], two_emb_layer=two_emb_layer)
    _, _, scale, _ = A.ERES2NET_ARCHS[arch]

    def bn(p, v):
        return F.batch_norm(v, sd[p + ".running_mean"], sd[p + ".running_var"], sd[p + ".weight"], sd[p + ".bias"],
                            False, 0.0, 1e-5)

    def act(v):
        return v.clamp(0.0, 20.0) if clamp else v.clamp_min(0.0)

    def aff(p, a, b):
        h = F.conv2d(torch.cat((a, b), 1), sd[p + ".local_att.0.weight"], sd[p + ".local_att.0.bias"])
        h = F.silu(bn(p + ".local_att.1", h))
        g = 1.0 + torch.tanh(bn(p + ".local_att.4", F.conv2d(h, sd[p + ".local_att.3.weight"],
                                                              sd[p + ".local_att.3.bias"])))
        return a * g + b * (2.0 - g)

    inter = {}
    out = F.relu(bn("bn1", F.conv2d(x.transpose(1, 2).unsqueeze(1), sd["conv1.weight"], padding=1)))
    inter["stem"] = out
    for p, _, _, w, stride, use_aff, has_sc in A.eres2net_blocks(spec):
        y = act(bn(p + ".bn1", F.conv2d(out, sd[p + ".conv1.weight"], stride=stride)))
        spx = torch.split(y, w, 1)
        parts = []
        sp = None
        for i in range(scale):
            if i == 0:
                sp = spx[0]
            elif use_aff:
                sp = aff(f"{p}.fuse_models.{i - 1}", sp, spx[i])
            else:
                sp = sp + spx[i]
            if use_aff:
                cw, cb = (p + ".conv2_1", p + ".bn2_1") if i == 0 else (f"{p}.convs.{i - 1}", f"{p}.bns.{i - 1}")
            else:
                cw, cb = f"{p}.convs.{i}", f"{p}.bns.{i}"
            sp = act(bn(cb, F.conv2d(sp, sd[cw + ".weight"], padding=1)))
            parts.append(sp)
        y = bn(p + ".bn3", F.conv2d(torch.cat(parts, 1), sd[p + ".conv3.weight"]))
        res = out
        if has_sc:
            res = bn(p + ".shortcut.1", F.conv2d(out, sd[p + ".shortcut.0.weight"], stride=stride))
        out = act(y + res)
        inter[p.split(".")[0]] = out  # the stage's last block stays
    fuse = inter["layer1"]
    for i, name in enumerate(("fuse_mode12", "fuse_mode123", "fuse_mode1234"), 1):
        down = F.conv2d(fuse, sd[f"layer{i}_downsample.weight"], stride=2, padding=1)
        fuse = aff(name, inter[f"layer{i + 1}"], down)
        inter[f"down{i}"] = down
        inter[name.replace("_mode", "")] = fuse
    # TSTP over (B, C, F, T) flattened channel-major (C, F): mean | unbiased std
    v = fuse.reshape(fuse.shape[0], -1, fuse.shape[3])
    stats = torch.cat((v.mean(-1), torch.sqrt(v.var(-1, unbiased=True) + 1e-7)), 1)
    emb = F.linear(stats, sd["seg_1.weight"], sd["seg_1.bias"])
    if two_emb_layer:
        r = F.relu(emb)
        r = (r - sd["seg_bn_1.running_mean"]) / torch.sqrt(sd["seg_bn_1.running_var"] + 1e-5)
        emb = F.linear(r, sd["seg_2.weight"], sd["seg_2.bias"])
    return (emb, inter) if taps else emb
