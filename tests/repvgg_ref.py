"""RepVGG (the REPVGG_* names, RepVGG and RepSPK blocks) restated on torch-CPU from the model's description:
the project's own oracle for the HIP path, in both checkpoint forms.

    forward(x, sd, arch, ...) -> embedding [B][embed_dim]  (and the stage outputs with taps=True)

x: (B, T, feat_dim) features, sd: state dict keyed by the reference names (numpy or torch).  The form is
read off the keys: with `stage0.rbr_reparam.weight` a block is relu(conv_kxk(x) + bias), k = 3 or 5 with
padding k // 2; else it is relu(bn(conv3x3(x)) + bn(branch(x)) + bn_identity(x)) with branch = the 1x1 conv
(RepVGG) or the dilation-2 3x3 conv with padding 2 (RepSPK), eval-mode BatchNorms applied as they are, in
the dtype asked for.  macs=True also returns the multiply-accumulates of every conv / linear of one
utterance, counted from the shapes of the calls made here (25 taps for a deploy-form RepSPK block)."""
import torch
import torch.nn.functional as F

from wespeaker_hubert_amd import arch as A

TAPS = ("stage0", "stage1", "stage2", "stage3", "stage4")


def forward(x, sd, arch="REPVGG_TINY_A0", dtype=torch.float32, taps=False, macs=False):
    sd = {k: torch.as_tensor(v).to(dtype) for k, v in sd.items() if not k.endswith("num_batches_tracked")}
    x = torch.as_tensor(x).to(dtype)
    deploy = "stage0.rbr_reparam.weight" in sd
    spec = A.make_spec(arch, feat_dim=x.shape[2], embed_dim=sd["seg.weight"].shape[0], deploy=deploy)
    spk = A.repvgg_kernel_size(spec) == 5
    count = [0]

    def conv(v, w, **kw):
        o = F.conv2d(v, w, **kw)
        count[0] += o.shape[2] * o.shape[3] * w.numel()  # per utterance
        return o

    def bn(p, v):
        return F.batch_norm(v, sd[p + ".running_mean"], sd[p + ".running_var"], sd[p + ".weight"], sd[p + ".bias"],
                            False, 0.0, 1e-5)

    inter = {}
    out = x.transpose(1, 2).unsqueeze(1)  # (B, T, F) -> (B, 1, F, T)
    for p, stage, _, _, stride, has_id in A.repvgg_blocks(spec):
        if deploy:
            w = sd[p + ".rbr_reparam.weight"]
            y = conv(out, w, bias=sd[p + ".rbr_reparam.bias"], stride=stride, padding=w.shape[-1] // 2)
        else:
            y = bn(p + ".rbr_dense.bn", conv(out, sd[p + ".rbr_dense.conv.weight"], stride=stride, padding=1))
            if spk:
                y = y + bn(p + ".rbr_dense_dilation.bn",
                           conv(out, sd[p + ".rbr_dense_dilation.conv.weight"], stride=stride, padding=2, dilation=2))
            else:
                y = y + bn(p + ".rbr_1x1.bn", conv(out, sd[p + ".rbr_1x1.conv.weight"], stride=stride))
            if has_id:
                y = y + bn(p + ".rbr_identity", out)
        out = F.relu(y)
        inter[f"stage{stage}"] = out  # the stage's last block stays
    # TSTP over (B, C, F, T) flattened channel-major (C, F): mean | unbiased std
    v = out.reshape(out.shape[0], -1, out.shape[3])
    stats = torch.cat((v.mean(-1), torch.sqrt(v.var(-1, unbiased=True) + 1e-7)), 1)
    count[0] += sd["seg.weight"].numel()
    emb = F.linear(stats, sd["seg.weight"], sd["seg.bias"])
    ret = (emb,) + ((inter,) if taps else ()) + ((count[0],) if macs else ())
    return ret if len(ret) > 1 else emb
