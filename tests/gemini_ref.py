"""Gemini DF-ResNet restated on torch-CPU from the model's description: the project's own oracle for
the HIP path.  Eval-mode BatchNorms are applied as they are (no folding), in the dtype asked for.

    forward(x, sd, arch, ...) -> embedding [B][embed_dim]  (and the named intermediates with taps=True)

x: (B, T, feat_dim) features, sd: state dict keyed by the reference names (numpy or torch, on
any one device).  With two_emb_layer the result is embed_b (the reference's outputs[-1]).
"""
import torch
import torch.nn.functional as F

from wespeaker_hubert_amd import arch as A

TAPS = ("stem", "down1", "stage1", "down2", "stage2", "down3", "stage3", "down4", "stage4")


def forward(x, sd, arch="Gemini_DF_ResNet60", two_emb_layer=False, dtype=torch.float32, taps=False):
    sd = {k: torch.as_tensor(v).to(dtype) for k, v in sd.items()}
    x = torch.as_tensor(x).to(dtype)

    def bn(p, v):
        return F.batch_norm(v, sd[p + ".running_mean"], sd[p + ".running_var"], sd[p + ".weight"], sd[p + ".bias"],
                            False, 0.0, 1e-5)

    inter = {}
    out = x.transpose(1, 2).unsqueeze(1)  # (B, T, F) -> (B, 1, F, T)
    out = F.relu(bn("downsample_layers.0.1", F.conv2d(out, sd["downsample_layers.0.0.weight"], padding=1)))
    inter["stem"] = out
    for li, depth in enumerate(A.GEMINI_ARCHS[arch]):
        p = f"downsample_layers.{li + 1}"
        out = bn(p + ".1", F.conv2d(out, sd[p + ".0.weight"], stride=(2, A.GEMINI_STRIDE_T[li]), padding=1))
        inter[f"down{li + 1}"] = out
        for bi in range(depth):
            p = f"stages.{li}.{bi}"
            y = F.relu(bn(p + ".bn1", F.conv2d(out, sd[p + ".conv1.weight"])))
            y = F.relu(bn(p + ".bn2", F.conv2d(y, sd[p + ".conv2.weight"], padding=1, groups=y.shape[1])))
            y = bn(p + ".bn3", F.conv2d(y, sd[p + ".conv3.weight"]))
            out = F.relu(y + out)
        inter[f"stage{li + 1}"] = out
    # TSTP over (B, C, F, T) flattened channel-major (C, F): mean | unbiased std
    v = out.reshape(out.shape[0], -1, out.shape[3])
    stats = torch.cat((v.mean(-1), torch.sqrt(v.var(-1, unbiased=True) + 1e-7)), 1)
    emb = F.linear(stats, sd["seg_1.weight"], sd["seg_1.bias"])
    if two_emb_layer:
        r = F.relu(emb)
        r = (r - sd["seg_bn_1.running_mean"]) / torch.sqrt(sd["seg_bn_1.running_var"] + 1e-5)
        emb = F.linear(r, sd["seg_2.weight"], sd["seg_2.bias"])
    return (emb, inter) if taps else emb
