"""Architecture registry: names, hyper-parameters and state_dict layout.

Mirrors `get_speaker_model(name)(**model_args)` (wespeaker/models/speaker_model.py:30-57)
for the backbones on the north-star path, and reproduces the exact state_dict
key/shape list of the reference modules so an `avg_model.pt` trained with the
reference loads unchanged (`load_checkpoint(strict=False)`,
wespeaker/utils/checkpoint.py:20-27).
"""
from __future__ import annotations

from dataclasses import dataclass, field
from typing import List, Tuple

ParamList = List[Tuple[str, Tuple[int, ...]]]

ECAPA_ARCHS = {
    # name: (channels, global_context_att) — ecapa_tdnn.py:237-274
    "ECAPA_TDNN_c512": (512, False),
    "ECAPA_TDNN_GLOB_c512": (512, True),
    "ECAPA_TDNN_c1024": (1024, False),
    "ECAPA_TDNN_GLOB_c1024": (1024, True),
}
RESNET_ARCHS = {
    # name: (block, num_blocks) — resnet.py:207-260
    "ResNet18": ("basic", (2, 2, 2, 2)),
    "ResNet34": ("basic", (3, 4, 6, 3)),
    "ResNet50": ("bottleneck", (3, 4, 6, 3)),
    "ResNet101": ("bottleneck", (3, 4, 23, 3)),
    "ResNet152": ("bottleneck", (3, 8, 36, 3)),
    "ResNet221": ("bottleneck", (6, 16, 48, 3)),
    "ResNet293": ("bottleneck", (10, 20, 64, 3)),
}

SIMAM_ARCHS = {
    # name: num_blocks of SimAMBasicBlock — samresnet.py:115-121, 124-166
    "SimAM_ResNet34_ASP": (3, 4, 6, 3),
    "SimAM_ResNet100_ASP": (6, 16, 24, 3),
}

CAMPP_ARCHS = {
    # name: (dense layers, dilation) per block — campplus.py:333-380 (kernel 3, growth 32, bn_size 4)
    "CAMPPlus": ((12, 24, 16), (1, 2, 2)),
}
CAMPP_SEG = 100  # CAMLayer.seg_pooling's segment length

ERES2NET_ARCHS = {
    # name: (m_channels, baseWidth, scale, expansion) — eres2net.py:394-430, num_blocks (3, 4, 6, 3)
    "ERes2Net34_Base": (32, 32, 2, 2),
    "ERes2Net34_Large": (64, 32, 2, 2),
    "ERes2Net34_aug": (64, 24, 3, 4),
}
ERES2NET_BLOCKS = (3, 4, 6, 3)

RES2NET_ARCHS = {
    # name: m_channels — res2net.py:192-211; BasicBlockRes2Net: expansion 2, baseWidth 32, scale 2 (the
    # constructors cannot change any of them), num_blocks (3, 4, 6, 3)
    "Res2Net34_Base": 32,
    "Res2Net34_Large": 64,
}
RES2NET_BLOCKS = (3, 4, 6, 3)
RES2NET_EXPANSION, RES2NET_SCALE = 2, 2

GEMINI_ARCHS = {
    # name: depths — gemini_dfresnet.py:145-178 (the downsample layers count as layers)
    "Gemini_DF_ResNet60": (3, 3, 9, 3),
    "Gemini_DF_ResNet114": (3, 3, 27, 3),
    "Gemini_DF_ResNet183": (3, 8, 45, 3),
    "Gemini_DF_ResNet237": (3, 8, 63, 3),
}
GEMINI_DIMS = (32, 32, 64, 128, 256)
GEMINI_STRIDE_T = (1, 2, 1, 1)  # Golden Gemini T14c: the frequency stride is 2 at every level

REDIMNET_ARCHS = {
    # name: (C, group_divisor, stages) with a stage = (frequency stride, 2-D ConvNeXt blocks, 1-D block
    # reduction 1152 / hC) — redimnet.py:924-947: convnext_like 2-D blocks, "conv+att" 1-D blocks
    "ReDimNetB2": (16, 4, ((1, 2, 12), (2, 2, 12), (1, 3, 12), (2, 4, 8), (1, 4, 8), (2, 4, 4))),
}
# the constructors the path refuses by name (other block types, group sizes, a stride-3 stage)
REDIMNET_OTHERS = ("ReDimNetB0", "ReDimNetB1", "ReDimNetB3", "ReDimNetB4", "ReDimNetB5", "ReDimNetB6")
REDIMNET_FEAT = 72
REDIMNET_DW_KERNELS = (7, 19, 31, 59)  # the four depthwise convs of a 1-D block (redimnet.py:584-607)
REDIMNET_HEADS = 4

REPVGG_ARCHS = {
    # name: (block kind, blocks per stage, stage-0 width, stage widths) — repvgg.py:602-747.  Strides are
    # (1, 1, 2, 2, 2) throughout; stage-0 width = min(64, int(64 * width_multiplier[0])); a RepSPK block
    # (the *_RSBB_* names) has a dilation-2 3x3 branch where a RepVGG block has its 1x1 branch
    "REPVGG_TINY_A0": ("RepVGG", (3, 4, 23, 3), 32, (32, 64, 128, 256)),
    "REPVGG_TINY_RSBB_A0": ("RepSPK", (3, 4, 23, 3), 32, (32, 64, 128, 256)),
    "REPVGG_A0": ("RepVGG", (2, 4, 14, 1), 48, (48, 96, 192, 1280)),
    "REPVGG_RSBB_A0": ("RepSPK", (2, 4, 14, 1), 48, (48, 96, 192, 1280)),
    "REPVGG_A1": ("RepVGG", (2, 4, 14, 1), 64, (64, 128, 256, 1280)),
    "REPVGG_A2": ("RepVGG", (2, 4, 14, 1), 64, (96, 192, 384, 1408)),
    "REPVGG_RSBB_A2": ("RepSPK", (2, 4, 14, 1), 64, (96, 192, 384, 1408)),
    "REPVGG_B0": ("RepVGG", (4, 6, 16, 1), 64, (64, 128, 256, 1280)),
    "REPVGG_RSBB_B0": ("RepSPK", (4, 6, 16, 1), 64, (64, 128, 256, 1280)),
}
# the constructors the path refuses by name, with the reason
REPVGG_OTHERS = {
    **{n: "stage-4 widths of 2048 / 2560" for n in ("REPVGG_B1", "REPVGG_B2", "REPVGG_B3")},
    **{n: "grouped convs" for n in ("REPVGG_B1g2", "REPVGG_B1g4", "REPVGG_B2g2", "REPVGG_B2g4", "REPVGG_B3g2",
                                    "REPVGG_B3g4")},
    "REPVGG_D2SE": "grouped convs and the 2-D SE block",
}
REPVGG_STRIDES = (1, 2, 2, 2)  # of stages 1..4 (stage0: 1)
# The 17 live taps (kf, kt) of a folded RepSPK 5x5 kernel, row-major: {kf, kt both even} (the dilated 3x3) and
# {1 <= kf, kt <= 3} (the plain 3x3), sharing the centre.  The other eight are structurally zero.
RSBB_LIVE_TAPS = tuple((kf, kt) for kf in range(5) for kt in range(5)
                       if (kf % 2 == 0 and kt % 2 == 0) or (1 <= kf <= 3 and 1 <= kt <= 3))
RSBB_DEAD_TAPS = tuple((kf, kt) for kf in range(5) for kt in range(5) if (kf, kt) not in RSBB_LIVE_TAPS)

XVEC_ARCHS = {
    # name: default pooling_func — tdnn.py:57-118, xi_vector.py XI_VEC_XVEC
    "XVEC": "TSTP",
    "XI_VEC_XVEC": "XI",
}
XVEC_HID, XVEC_STATS = 512, 1500
# (kernel, dilation) of frame_1..5: unpadded convs, T' = T - 14
XVEC_FRAMES = ((5, 1), (3, 2), (3, 3), (1, 1), (1, 1))
XVEC_SHRINK = sum((k - 1) * d for k, d in XVEC_FRAMES)
XI_HIDDEN = 256  # pooling_layers.py class XI: hidden_size 256, stddev False (the constructors cannot change either)
XI_ECAPA_ARCHS = {
    # name: channels — xi_vector.py: ECAPA_TDNN(pooling_func='XI'), no global context
    "XI_VEC_ECAPA_TDNN_c512": 512,
    "XI_VEC_ECAPA_TDNN_c1024": 1024,
}


@dataclass
class ModelSpec:
    arch: str
    feat_dim: int = 80
    embed_dim: int = 192
    pooling_func: str = "ASTP"
    emb_bn: bool = False
    two_emb_layer: bool = False
    m_channels: int = 32
    extra: dict = field(default_factory=dict)
    deploy: bool = False  # RepVGG: the state_dict layout (False: training branches, True: rbr_reparam)

    @property
    def family(self) -> str:
        if self.arch in RES2NET_ARCHS:  # before anything that matches by prefix
            return "res2net"
        if self.arch in REPVGG_ARCHS:
            return "repvgg"
        if self.arch.startswith("ECAPA_TDNN") or self.arch in XI_ECAPA_ARCHS:
            return "ecapa"
        if self.arch in XVEC_ARCHS:
            return "xvec"
        if self.arch.startswith("ResNet"):
            return "resnet"
        if self.arch.startswith("SimAM_ResNet"):
            return "simam"
        if self.arch in CAMPP_ARCHS:
            return "campplus"
        if self.arch in ERES2NET_ARCHS:
            return "eres2net"
        if self.arch in GEMINI_ARCHS:
            return "gemini"
        if self.arch in REDIMNET_ARCHS:
            return "redimnet"
        raise KeyError(self.arch)


def check_arch(arch: str) -> None:
    """Unknown names raise (the reference prints and exit(1)s, speaker_model.py:55-57)."""
    if arch in REDIMNET_OTHERS:
        raise NotImplementedError(f"{arch}: the ReDimNet path implements ReDimNetB2 (the voxceleb/v2 recipe); the other "
                                  "sizes need other block types, group sizes and a stride-3 stage")
    if arch in REPVGG_OTHERS:
        raise NotImplementedError(f"{arch}: the RepVGG path implements the TINY_A0 / A0 / A1 / A2 / B0 sizes and their "
                                  f"RSBB variants; {arch} needs {REPVGG_OTHERS[arch]}")
    known = (ECAPA_ARCHS, RESNET_ARCHS, SIMAM_ARCHS, CAMPP_ARCHS, ERES2NET_ARCHS, GEMINI_ARCHS, XVEC_ARCHS,
             XI_ECAPA_ARCHS, REDIMNET_ARCHS, RES2NET_ARCHS, REPVGG_ARCHS)
    if not any(arch in k for k in known):
        raise KeyError(f"{arch} not found !!! (supported: {sum((sorted(k) for k in known), [])})")


def make_spec(arch: str, **model_args) -> ModelSpec:
    """`get_speaker_model(arch)(**model_args)` analogue (speaker_model.py:30-57)."""
    check_arch(arch)
    kw = dict(model_args)
    if arch in XVEC_ARCHS:
        # XVEC(feat_dim=40, hid_dim=512, stats_dim=1500, embed_dim=512, pooling_func='TSTP');
        # XI_VEC_XVEC(feat_dim, embed_dim, pooling_func='XI') builds the same class
        spec = ModelSpec(arch=arch, feat_dim=int(kw.pop("feat_dim", 40)), embed_dim=int(kw.pop("embed_dim", 512)),
                         pooling_func=kw.pop("pooling_func", XVEC_ARCHS[arch]))
        if spec.pooling_func not in ("TSTP", "XI"):
            raise NotImplementedError("XVEC path implements TSTP and XI pooling")
        for key in ("emb_bn", "two_emb_layer"):  # tdnn.py's constructor has neither (a TypeError there too)
            if key in kw:
                raise TypeError(f"XVEC has no {key}")
        for key, want in (("hid_dim", XVEC_HID), ("stats_dim", XVEC_STATS)):
            if kw.pop(key, want) != want:
                raise NotImplementedError(f"XVEC path implements {key}={want} (the recipe configuration)")
        if spec.feat_dim < 4 or spec.feat_dim % 4:
            raise ValueError("XVEC feat_dim must be a positive multiple of 4")
        spec.extra = kw
        return spec
    if arch in REDIMNET_ARCHS:
        # ReDimNetB2(feat_dim=72, embed_dim=192, pooling_func='ASTP', two_emb_layer=False) (redimnet.py:924)
        spec = ModelSpec(arch=arch, feat_dim=int(kw.pop("feat_dim", REDIMNET_FEAT)), embed_dim=int(kw.pop("embed_dim", 192)),
                         pooling_func=kw.pop("pooling_func", "ASTP"),
                         two_emb_layer=bool(kw.pop("two_emb_layer", False)))
        if "emb_bn" in kw:  # the constructor has none (a TypeError there too)
            raise TypeError("ReDimNetB2 has no emb_bn")
        if spec.pooling_func != "ASTP":
            raise NotImplementedError("ReDimNet path implements ASTP pooling (the recipe configuration)")
        if spec.feat_dim != REDIMNET_FEAT:
            raise ValueError("ReDimNet path implements feat_dim=72 (the recipe configuration: C * F = 1152)")
        spec.extra = kw
        return spec
    if arch in XI_ECAPA_ARCHS:
        # XI_VEC_ECAPA_TDNN_c*(feat_dim, embed_dim, pooling_func='XI', emb_bn=False): no defaults in the
        # reference; the project's ECAPA defaults
        spec = ModelSpec(arch=arch, feat_dim=int(kw.pop("feat_dim", 80)), embed_dim=int(kw.pop("embed_dim", 192)),
                         pooling_func=kw.pop("pooling_func", "XI"), emb_bn=bool(kw.pop("emb_bn", False)))
        if spec.pooling_func != "XI":
            raise NotImplementedError("XI_VEC_ECAPA_TDNN path implements XI pooling (ASTP: the ECAPA_TDNN_* names)")
        if "two_emb_layer" in kw:  # xi_vector.py's factories do not take it (a TypeError there too)
            raise TypeError("XI_VEC_ECAPA_TDNN has no two_emb_layer")
        spec.extra = kw
        return spec
    if arch in GEMINI_ARCHS:
        # Gemini_DF_ResNet*(feat_dim, embed_dim, pooling_func='TSTP', two_emb_layer=False); the class
        # defaults are feat_dim 40 / embed_dim 128 (gemini_dfresnet.py:53-59)
        spec = ModelSpec(arch=arch, feat_dim=int(kw.pop("feat_dim", 40)), embed_dim=int(kw.pop("embed_dim", 128)),
                         pooling_func=kw.pop("pooling_func", "TSTP"),
                         two_emb_layer=bool(kw.pop("two_emb_layer", False)))
        if spec.pooling_func != "TSTP":
            raise NotImplementedError("Gemini DF-ResNet path implements TSTP pooling (the recipe configuration)")
        if spec.feat_dim < 16 or spec.feat_dim % 16:
            # gemini_dfresnet.py:63 sizes seg_1 for int(feat_dim / 16) rows while level 4 keeps ceil(feat_dim / 16)
            raise ValueError("Gemini DF-ResNet feat_dim must be a positive multiple of 16")
        spec.extra = kw
        return spec
    if arch in REPVGG_ARCHS:
        # REPVGG_*(feat_dim, embed_dim, pooling_func='TSTP', deploy=False, use_se=False): no defaults for the
        # first two in the reference; 80 / 256 (the recipes' values)
        spec = ModelSpec(arch=arch, feat_dim=int(kw.pop("feat_dim", 80)), embed_dim=int(kw.pop("embed_dim", 256)),
                         pooling_func=kw.pop("pooling_func", "TSTP"), deploy=bool(kw.pop("deploy", False)))
        for key in ("emb_bn", "two_emb_layer"):  # the constructors have neither (a TypeError there too)
            if key in kw:
                raise TypeError(f"RepVGG has no {key}")
        if kw.pop("use_se", False):
            raise NotImplementedError("RepVGG path implements use_se=False (the recipe configuration); the 2-D SE block "
                                      "is not implemented")
        if spec.pooling_func != "TSTP":
            raise NotImplementedError("RepVGG path implements TSTP pooling (the recipe configuration)")
        if spec.feat_dim < 8 or spec.feat_dim % 8:
            # repvgg.py:520 sizes the pooling for int(feat_dim / 8) rows while stage 4 keeps ceil(feat_dim / 8)
            raise ValueError("RepVGG feat_dim must be a positive multiple of 8")
        if spec.embed_dim < 1:
            raise ValueError("RepVGG embed_dim must be positive")
        spec.extra = kw
        return spec
    if arch in RES2NET_ARCHS:
        # Res2Net34_*(feat_dim, embed_dim, pooling_func='TSTP', two_emb_layer=False): no defaults for the
        # first two in the reference; the project's 80 / 192
        spec = ModelSpec(arch=arch, feat_dim=int(kw.pop("feat_dim", 80)), embed_dim=int(kw.pop("embed_dim", 192)),
                         pooling_func=kw.pop("pooling_func", "TSTP"),
                         two_emb_layer=bool(kw.pop("two_emb_layer", False)), m_channels=RES2NET_ARCHS[arch])
        if "emb_bn" in kw:  # the constructor has none (a TypeError there too)
            raise TypeError("Res2Net has no emb_bn")
        if spec.pooling_func != "TSTP":
            raise NotImplementedError("Res2Net path implements TSTP pooling (the recipe configuration)")
        if spec.feat_dim < 8 or spec.feat_dim % 8:
            # res2net.py:110 sizes seg_1 for int(feat_dim / 8) rows while stage 4 keeps ceil(feat_dim / 8)
            raise ValueError("Res2Net feat_dim must be a positive multiple of 8")
        spec.extra = kw
        return spec
    if arch in ERES2NET_ARCHS:
        # ERes2Net34_*(feat_dim, embed_dim, pooling_func='TSTP', two_emb_layer=False)
        spec = ModelSpec(arch=arch, feat_dim=int(kw.pop("feat_dim", 80)), embed_dim=int(kw.pop("embed_dim", 192)),
                         pooling_func=kw.pop("pooling_func", "TSTP"),
                         two_emb_layer=bool(kw.pop("two_emb_layer", False)), m_channels=ERES2NET_ARCHS[arch][0])
        if spec.pooling_func != "TSTP":
            raise NotImplementedError("ERes2Net path implements TSTP pooling (the recipe configuration)")
        if spec.feat_dim < 8 or spec.feat_dim % 8:
            # eres2net.py:261 sizes seg_1 for int(feat_dim / 8) rows while stage 4 keeps ceil(feat_dim / 8)
            raise ValueError("ERes2Net feat_dim must be a positive multiple of 8")
        spec.extra = kw
        return spec
    if arch in CAMPP_ARCHS:
        # CAMPPlus(feat_dim=80, embed_dim=512, pooling_func='TSTP', growth_rate=32, bn_size=4,
        #          init_channels=128, config_str='batchnorm-relu')
        spec = ModelSpec(arch=arch, feat_dim=int(kw.pop("feat_dim", 80)), embed_dim=int(kw.pop("embed_dim", 512)),
                         pooling_func=kw.pop("pooling_func", "TSTP"))
        if spec.pooling_func != "TSTP":
            raise NotImplementedError("CAMPPlus path implements TSTP pooling (the hub configuration)")
        if spec.feat_dim < 8 or spec.feat_dim % 8:
            raise ValueError("CAMPPlus feat_dim must be a positive multiple of 8")
        for key, want in (("growth_rate", 32), ("bn_size", 4), ("init_channels", 128),
                          ("config_str", "batchnorm-relu")):
            if kw.pop(key, want) != want:
                raise NotImplementedError(f"CAMPPlus path implements {key}={want!r} (the hub configuration)")
        spec.extra = kw
        return spec
    if arch in SIMAM_ARCHS:
        # SimAM_ResNet*_ASP(in_planes=64, embed_dim=256, acoustic_dim=80, dropout=0)
        spec = ModelSpec(arch=arch, feat_dim=int(kw.pop("acoustic_dim", 80)),
                         embed_dim=int(kw.pop("embed_dim", 256)), pooling_func="ASP",
                         m_channels=int(kw.pop("in_planes", 64)))
        kw.pop("dropout", None)  # eval: nn.Dropout is the identity
        spec.extra = kw
        return spec
    spec = ModelSpec(arch=arch,
                     feat_dim=int(kw.pop("feat_dim", 80 if arch.startswith("ECAPA") else 40)),
                     embed_dim=int(kw.pop("embed_dim", 192 if arch.startswith("ECAPA") else 128)),
                     pooling_func=kw.pop("pooling_func", "ASTP" if arch.startswith("ECAPA") else "TSTP"),
                     emb_bn=bool(kw.pop("emb_bn", False)),
                     two_emb_layer=bool(kw.pop("two_emb_layer", False)))
    if spec.family == "ecapa" and spec.pooling_func != "ASTP":
        raise NotImplementedError("ECAPA path implements ASTP pooling (the north-star config)")
    if spec.family == "resnet" and spec.pooling_func != "TSTP":
        raise NotImplementedError("ResNet path implements TSTP pooling (the north-star config)")
    spec.extra = kw
    return spec


def _bn(p: str, c: int) -> ParamList:
    return [(p + ".weight", (c,)), (p + ".bias", (c,)), (p + ".running_mean", (c,)),
            (p + ".running_var", (c,)), (p + ".num_batches_tracked", ())]


def xi_params(p: str, dim: int) -> ParamList:
    """state_dict layout of the XI pooling layer (pooling_layers.py class XI) over `dim` channels."""
    out: ParamList = [(p + ".prior_mean", (1, dim)), (p + ".prior_logprec", (1, dim)),
                      (p + ".lin1_relu_bn.0.weight", (XI_HIDDEN, dim, 1)), (p + ".lin1_relu_bn.0.bias", (XI_HIDDEN,))]
    out += _bn(p + ".lin1_relu_bn.2", XI_HIDDEN)
    out += [(p + ".lin2.weight", (dim, XI_HIDDEN, 1)), (p + ".lin2.bias", (dim,))]
    return out


def xvec_handle_arch(spec: ModelSpec) -> str:
    """The library's arch string of an x-vector spec: the C ABI has no pooling argument, so the name
    carries it (XVEC = TSTP, XI_VEC_XVEC = XI), whichever constructor the caller used."""
    return "XI_VEC_XVEC" if spec.pooling_func == "XI" else "XVEC"


def xvec_min_frames(spec: ModelSpec) -> int:
    """T' = T - 14 frames reach the pooling: XI needs one, TSTP's unbiased variance two."""
    return XVEC_SHRINK + (1 if spec.pooling_func == "XI" else 2)


def xvec_params(spec: ModelSpec) -> ParamList:
    """state_dict layout of XVEC (tdnn.py:23-91): five TDNN layers whose BatchNorm has no affine
    (running statistics only), the pooling layer's parameters (XI only), seg_1, seg_bn_1, seg_2."""
    out: ParamList = []
    cin = spec.feat_dim
    for i, (k, _) in enumerate(XVEC_FRAMES, 1):
        cout = XVEC_STATS if i == 5 else XVEC_HID
        p = f"frame_{i}"
        out += [(p + ".conv_1d.weight", (cout, cin, k)), (p + ".conv_1d.bias", (cout,)),
                (p + ".bn.running_mean", (cout,)), (p + ".bn.running_var", (cout,)), (p + ".bn.num_batches_tracked", ())]
        cin = cout
    xi = spec.pooling_func == "XI"
    if xi:
        out += xi_params("pool", XVEC_STATS)
    E = spec.embed_dim
    out += [("seg_1.weight", (E, XVEC_STATS * (1 if xi else 2))), ("seg_1.bias", (E,)),
            ("seg_bn_1.running_mean", (E,)), ("seg_bn_1.running_var", (E,)), ("seg_bn_1.num_batches_tracked", ()),
            ("seg_2.weight", (E, E)), ("seg_2.bias", (E,))]
    return out


def ecapa_params(spec: ModelSpec) -> ParamList:
    """state_dict layout of ECAPA_TDNN (ecapa_tdnn.py:160-206); the XI_VEC_ECAPA_TDNN_* names carry
    the XI pooling layer and a 1536-wide head."""
    xi = spec.arch in XI_ECAPA_ARCHS
    C, glob = (XI_ECAPA_ARCHS[spec.arch], False) if xi else ECAPA_ARCHS[spec.arch]
    w = C // 8
    out: ParamList = [("layer1.conv.weight", (C, spec.feat_dim, 5)), ("layer1.conv.bias", (C,))]
    out += _bn("layer1.bn", C)
    for li in (2, 3, 4):
        p = f"layer{li}.se_res2block"
        out += [(f"{p}.0.conv.weight", (C, C, 1)), (f"{p}.0.conv.bias", (C,))] + _bn(f"{p}.0.bn", C)
        for i in range(7):
            out += [(f"{p}.1.convs.{i}.weight", (w, w, 3)), (f"{p}.1.convs.{i}.bias", (w,))]
        for i in range(7):
            out += _bn(f"{p}.1.bns.{i}", w)
        out += [(f"{p}.2.conv.weight", (C, C, 1)), (f"{p}.2.conv.bias", (C,))] + _bn(f"{p}.2.bn", C)
        out += [(f"{p}.3.linear1.weight", (128, C)), (f"{p}.3.linear1.bias", (128,)),
                (f"{p}.3.linear2.weight", (C, 128)), (f"{p}.3.linear2.bias", (C,))]
    out += [("conv.weight", (1536, 3 * C, 1)), ("conv.bias", (1536,))]
    if xi:
        out += xi_params("pool", 1536)
    else:
        out += [("pool.linear1.weight", (128, 1536 * (3 if glob else 1), 1)), ("pool.linear1.bias", (128,)),
                ("pool.linear2.weight", (1536, 128, 1)), ("pool.linear2.bias", (1536,))]
    pooled = 1536 if xi else 3072
    out += _bn("bn", pooled)
    out += [("linear.weight", (spec.embed_dim, pooled)), ("linear.bias", (spec.embed_dim,))]
    if spec.emb_bn:
        out += _bn("bn2", spec.embed_dim)
    return out


def resnet_params(spec: ModelSpec) -> ParamList:
    """state_dict layout of ResNet (resnet.py:110-169)."""
    kind, nblocks = RESNET_ARCHS[spec.arch]
    m = spec.m_channels
    exp = 1 if kind == "basic" else 4
    out: ParamList = [("conv1.weight", (m, 1, 3, 3))] + _bn("bn1", m)
    in_planes = m
    for li, n in enumerate(nblocks):
        planes = m * (2 ** li)
        for bi in range(n):
            stride = 2 if (li > 0 and bi == 0) else 1
            p = f"layer{li + 1}.{bi}"
            if kind == "basic":
                out += [(p + ".conv1.weight", (planes, in_planes, 3, 3))] + _bn(p + ".bn1", planes)
                out += [(p + ".conv2.weight", (planes, planes, 3, 3))] + _bn(p + ".bn2", planes)
            else:
                out += [(p + ".conv1.weight", (planes, in_planes, 1, 1))] + _bn(p + ".bn1", planes)
                out += [(p + ".conv2.weight", (planes, planes, 3, 3))] + _bn(p + ".bn2", planes)
                out += [(p + ".conv3.weight", (planes * 4, planes, 1, 1))] + _bn(p + ".bn3", planes * 4)
            if stride != 1 or in_planes != exp * planes:
                out += [(p + ".shortcut.0.weight", (exp * planes, in_planes, 1, 1))]
                out += _bn(p + ".shortcut.1", exp * planes)
            in_planes = planes * exp
    stats_dim = int(spec.feat_dim / 8) * m * 8 * exp
    out += [("seg_1.weight", (spec.embed_dim, stats_dim * 2)), ("seg_1.bias", (spec.embed_dim,))]
    if spec.two_emb_layer:
        out += [("seg_bn_1.running_mean", (spec.embed_dim,)), ("seg_bn_1.running_var", (spec.embed_dim,)),
                ("seg_bn_1.num_batches_tracked", ()),
                ("seg_2.weight", (spec.embed_dim, spec.embed_dim)), ("seg_2.bias", (spec.embed_dim,))]
    return out


def simam_params(spec: ModelSpec) -> ParamList:
    """state_dict layout of SimAM_ResNet*_ASP (samresnet.py:72-166, ASP pooling_layers.py:151-164)."""
    m = spec.m_channels
    out: ParamList = [("front.conv1.weight", (m, 1, 3, 3))] + _bn("front.bn1", m)
    in_planes = m
    for li, n in enumerate(SIMAM_ARCHS[spec.arch]):
        planes = m * (2 ** li)
        for bi in range(n):
            stride = 2 if (li > 0 and bi == 0) else 1
            p = f"front.layer{li + 1}.{bi}"
            out += [(p + ".conv1.weight", (planes, in_planes, 3, 3))] + _bn(p + ".bn1", planes)
            out += [(p + ".conv2.weight", (planes, planes, 3, 3))] + _bn(p + ".bn2", planes)
            if stride != 1 or in_planes != planes:
                out += [(p + ".downsample.0.weight", (planes, in_planes, 1, 1))] + _bn(p + ".downsample.1", planes)
            in_planes = planes
    cf = m * 8 * int(spec.feat_dim / 8)
    out += [("pooling.attention.0.weight", (128, cf, 1)), ("pooling.attention.0.bias", (128,))]
    out += _bn("pooling.attention.2", 128)
    out += [("pooling.attention.3.weight", (cf, 128, 1)), ("pooling.attention.3.bias", (cf,))]
    out += [("bottleneck.weight", (spec.embed_dim, 2 * cf)), ("bottleneck.bias", (spec.embed_dim,))]
    return out


def campplus_params(spec: ModelSpec) -> ParamList:
    """state_dict layout of CAMPPlus (campplus.py:245-396): FCM head, xvector.* dense TDNN."""
    layers, _ = CAMPP_ARCHS[spec.arch]
    out: ParamList = [("head.conv1.weight", (32, 1, 3, 3))] + _bn("head.bn1", 32)
    for stage in (1, 2):
        for bi in (0, 1):
            p = f"head.layer{stage}.{bi}"
            out += [(p + ".conv1.weight", (32, 32, 3, 3))] + _bn(p + ".bn1", 32)
            out += [(p + ".conv2.weight", (32, 32, 3, 3))] + _bn(p + ".bn2", 32)
            if bi == 0:
                out += [(p + ".shortcut.0.weight", (32, 32, 1, 1))] + _bn(p + ".shortcut.1", 32)
    out += [("head.conv2.weight", (32, 32, 3, 3))] + _bn("head.bn2", 32)
    out += [("xvector.tdnn.linear.weight", (128, 32 * (spec.feat_dim // 8), 5))]
    out += _bn("xvector.tdnn.nonlinear.batchnorm", 128)
    ch = 128
    for b, n in enumerate(layers):
        for i in range(n):
            p = f"xvector.block{b + 1}.tdnnd{i + 1}"
            cin = ch + 32 * i
            out += _bn(p + ".nonlinear1.batchnorm", cin)
            out += [(p + ".linear1.weight", (128, cin, 1))]
            out += _bn(p + ".nonlinear2.batchnorm", 128)
            out += [(p + ".cam_layer.linear_local.weight", (32, 128, 3)),
                    (p + ".cam_layer.linear1.weight", (64, 128, 1)), (p + ".cam_layer.linear1.bias", (64,)),
                    (p + ".cam_layer.linear2.weight", (32, 64, 1)), (p + ".cam_layer.linear2.bias", (32,))]
        ch += 32 * n
        t = f"xvector.transit{b + 1}"
        out += _bn(t + ".nonlinear.batchnorm", ch) + [(t + ".linear.weight", (ch // 2, ch, 1))]
        ch //= 2
    out += _bn("xvector.out_nonlinear.batchnorm", ch)
    out += [("xvector.dense.linear.weight", (spec.embed_dim, 2 * ch, 1)),
            ("xvector.dense.nonlinear.batchnorm.running_mean", (spec.embed_dim,)),
            ("xvector.dense.nonlinear.batchnorm.running_var", (spec.embed_dim,)),
            ("xvector.dense.nonlinear.batchnorm.num_batches_tracked", ())]
    return out


def eres2net_blocks(spec: ModelSpec):
    """(prefix, in_planes, planes, width, stride, aff, has_shortcut) of every block (eres2net.py:106-352)."""
    m, base_width, scale, exp = ERES2NET_ARCHS[spec.arch]
    in_planes = m
    for li, n in enumerate(ERES2NET_BLOCKS):
        planes = m * (2 ** li)
        width = int(planes * base_width // 64)
        for bi in range(n):
            stride = 2 if (li > 0 and bi == 0) else 1
            yield (f"layer{li + 1}.{bi}", in_planes, planes, width, stride, li >= 2,
                   stride != 1 or in_planes != exp * planes)
            in_planes = exp * planes


def _aff(p: str, c: int) -> ParamList:
    h = c // 4
    return ([(p + ".local_att.0.weight", (h, 2 * c, 1, 1)), (p + ".local_att.0.bias", (h,))] + _bn(p + ".local_att.1", h)
            + [(p + ".local_att.3.weight", (c, h, 1, 1)), (p + ".local_att.3.bias", (c,))] + _bn(p + ".local_att.4", c))


def eres2net_params(spec: ModelSpec) -> ParamList:
    """state_dict layout of ERes2Net (eres2net.py:75-335): stem, the Res2 blocks (stages 3-4 with an
    AFF in front of every 3x3 conv but the first), the bottom-up downsample convs and AFFs, seg_1."""
    m, _, scale, exp = ERES2NET_ARCHS[spec.arch]
    out: ParamList = [("conv1.weight", (m, 1, 3, 3))] + _bn("bn1", m)
    for p, in_planes, planes, w, stride, aff, has_sc in eres2net_blocks(spec):
        out += [(p + ".conv1.weight", (w * scale, in_planes, 1, 1))] + _bn(p + ".bn1", w * scale)
        if aff:
            out += [(p + ".conv2_1.weight", (w, w, 3, 3))] + _bn(p + ".bn2_1", w)
            out += [(f"{p}.convs.{i}.weight", (w, w, 3, 3)) for i in range(scale - 1)]
            for i in range(scale - 1):
                out += _bn(f"{p}.bns.{i}", w)
            for i in range(scale - 1):
                out += _aff(f"{p}.fuse_models.{i}", w)
        else:
            out += [(f"{p}.convs.{i}.weight", (w, w, 3, 3)) for i in range(scale)]
            for i in range(scale):
                out += _bn(f"{p}.bns.{i}", w)
        out += [(p + ".conv3.weight", (planes * exp, w * scale, 1, 1))] + _bn(p + ".bn3", planes * exp)
        if has_sc:
            out += [(p + ".shortcut.0.weight", (planes * exp, in_planes, 1, 1))] + _bn(p + ".shortcut.1", planes * exp)
    c = m * exp
    out += [(f"layer{i}_downsample.weight", (c * 2 ** i, c * 2 ** (i - 1), 3, 3)) for i in (1, 2, 3)]
    for i, name in enumerate(("fuse_mode12", "fuse_mode123", "fuse_mode1234"), 1):
        out += _aff(name, c * 2 ** i)
    stats_dim = int(spec.feat_dim / 8) * m * 8 * exp
    out += [("seg_1.weight", (spec.embed_dim, stats_dim * 2)), ("seg_1.bias", (spec.embed_dim,))]
    if spec.two_emb_layer:
        out += [("seg_bn_1.running_mean", (spec.embed_dim,)), ("seg_bn_1.running_var", (spec.embed_dim,)),
                ("seg_bn_1.num_batches_tracked", ()),
                ("seg_2.weight", (spec.embed_dim, spec.embed_dim)), ("seg_2.bias", (spec.embed_dim,))]
    return out


def res2net_blocks(spec: ModelSpec):
    """(prefix, in_planes, planes, width, stride, has_shortcut) of every block (res2net.py:34-155)."""
    m, exp = RES2NET_ARCHS[spec.arch], RES2NET_EXPANSION
    in_planes = m
    for li, n in enumerate(RES2NET_BLOCKS):
        planes = m * (2 ** li)
        for bi in range(n):
            stride = 2 if (li > 0 and bi == 0) else 1
            yield (f"layer{li + 1}.{bi}", in_planes, planes, planes // 2, stride,
                   stride != 1 or in_planes != exp * planes)
            in_planes = exp * planes


def res2net_params(spec: ModelSpec) -> ParamList:
    """state_dict layout of Res2Net (res2net.py:34-147): stem, the blocks (conv1, the one 3x3 conv of the
    scale-2 chain, conv3, the projection shortcut of a stage's first block), seg_1 (+ seg_bn_1 / seg_2)."""
    m, exp = RES2NET_ARCHS[spec.arch], RES2NET_EXPANSION
    out: ParamList = [("conv1.weight", (m, 1, 3, 3))] + _bn("bn1", m)
    for p, in_planes, planes, w, stride, has_sc in res2net_blocks(spec):
        out += [(p + ".conv1.weight", (2 * w, in_planes, 1, 1))] + _bn(p + ".bn1", 2 * w)
        out += [(p + ".convs.0.weight", (w, w, 3, 3))] + _bn(p + ".bns.0", w)
        out += [(p + ".conv3.weight", (planes * exp, 2 * w, 1, 1))] + _bn(p + ".bn3", planes * exp)
        if has_sc:
            out += [(p + ".shortcut.0.weight", (planes * exp, in_planes, 1, 1))] + _bn(p + ".shortcut.1", planes * exp)
    stats_dim = int(spec.feat_dim / 8) * m * 8 * exp
    out += [("seg_1.weight", (spec.embed_dim, stats_dim * 2)), ("seg_1.bias", (spec.embed_dim,))]
    if spec.two_emb_layer:
        out += [("seg_bn_1.running_mean", (spec.embed_dim,)), ("seg_bn_1.running_var", (spec.embed_dim,)),
                ("seg_bn_1.num_batches_tracked", ()),
                ("seg_2.weight", (spec.embed_dim, spec.embed_dim)), ("seg_2.bias", (spec.embed_dim,))]
    return out


def repvgg_blocks(spec: ModelSpec):
    """(prefix, stage 0..4, cin, cout, stride, has_identity) of every block (repvgg.py:456-554); stage0 is
    the 1 -> C0 stem, itself a block of the family's kind."""
    _, nblocks, c0, widths = REPVGG_ARCHS[spec.arch]
    yield ("stage0", 0, 1, c0, 1, False)
    cin = c0
    for li, n in enumerate(nblocks):
        for bi in range(n):
            stride = REPVGG_STRIDES[li] if bi == 0 else 1
            yield (f"stage{li + 1}.{bi}", li + 1, cin, widths[li], stride, cin == widths[li] and stride == 1)
            cin = widths[li]


def repvgg_kernel_size(spec: ModelSpec) -> int:
    """Side of a block's folded kernel: 3 (RepVGG), 5 (RepSPK)."""
    return 5 if REPVGG_ARCHS[spec.arch][0] == "RepSPK" else 3


def repvgg_params(spec: ModelSpec) -> ParamList:
    """state_dict layout of RepVGG (repvgg.py:105-554) in the form `spec.deploy` selects.  Training form
    (avg_model.pt): per block the identity BatchNorm (where cin == cout and stride 1), rbr_dense.{conv, bn}
    and rbr_1x1.{conv, bn} (RepSPK: rbr_dense_dilation in its place).  Deploy form (convert_model.pt): per
    block rbr_reparam.{weight [cout, cin, k, k], bias}, k = 3 or 5.  Then seg."""
    spk = REPVGG_ARCHS[spec.arch][0] == "RepSPK"
    k = repvgg_kernel_size(spec)
    out: ParamList = []
    cout = 0
    for p, _, cin, cout, _, has_id in repvgg_blocks(spec):
        if spec.deploy:
            out += [(p + ".rbr_reparam.weight", (cout, cin, k, k)), (p + ".rbr_reparam.bias", (cout,))]
            continue
        if has_id:
            out += _bn(p + ".rbr_identity", cin)
        out += [(p + ".rbr_dense.conv.weight", (cout, cin, 3, 3))] + _bn(p + ".rbr_dense.bn", cout)
        if spk:
            out += [(p + ".rbr_dense_dilation.conv.weight", (cout, cin, 3, 3))] + _bn(p + ".rbr_dense_dilation.bn", cout)
        else:
            out += [(p + ".rbr_1x1.conv.weight", (cout, cin, 1, 1))] + _bn(p + ".rbr_1x1.bn", cout)
    stats_dim = cout * int(spec.feat_dim / 8)
    out += [("seg.weight", (spec.embed_dim, 2 * stats_dim)), ("seg.bias", (spec.embed_dim,))]
    return out


def repvgg_fold(spec: ModelSpec, state_dict) -> dict:
    """Training-form state_dict -> deploy-form state_dict (float32 numpy, repvgg_params(deploy=True) order),
    computed in float64.  Every branch's eval BatchNorm (eps 1e-5) is folded into its kernel,
        K' = K * g / sqrt(v + eps) per output channel,   b' = beta - mean * g / sqrt(v + eps),
    and the branches are summed into one k x k kernel: RepVGG (k = 3) the 3x3 kernel plus the 1x1 kernel at
    the centre tap; RepSPK (k = 5) the 3x3 kernel at the inner taps 1..3 plus the dilation-2 3x3 kernel at
    the even taps 0, 2, 4; the identity BatchNorm as a centre-tap diagonal.  The eight taps of a RepSPK
    kernel that no branch reaches are exact zeros."""
    import numpy as np

    def get(name):
        v = state_dict[name]
        if hasattr(v, "detach"):
            v = v.detach().cpu().numpy()
        return np.asarray(v, dtype=np.float64)

    def affine(p):
        t = get(p + ".weight") / np.sqrt(get(p + ".running_var") + 1e-5)
        return t, get(p + ".bias") - get(p + ".running_mean") * t

    spk = REPVGG_ARCHS[spec.arch][0] == "RepSPK"
    k = repvgg_kernel_size(spec)
    c = k // 2
    out = {}
    for p, _, cin, cout, _, has_id in repvgg_blocks(spec):
        kern = np.zeros((cout, cin, k, k), dtype=np.float64)
        t, bias = affine(p + ".rbr_dense.bn")
        kern[:, :, c - 1:c + 2, c - 1:c + 2] += get(p + ".rbr_dense.conv.weight") * t[:, None, None, None]
        if spk:
            t, b = affine(p + ".rbr_dense_dilation.bn")
            kern[:, :, ::2, ::2] += get(p + ".rbr_dense_dilation.conv.weight") * t[:, None, None, None]
        else:
            t, b = affine(p + ".rbr_1x1.bn")
            kern[:, :, c, c] += get(p + ".rbr_1x1.conv.weight")[:, :, 0, 0] * t[:, None]
        bias = bias + b
        if has_id:
            t, b = affine(p + ".rbr_identity")
            kern[np.arange(cout), np.arange(cin), c, c] += t
            bias = bias + b
        out[p + ".rbr_reparam.weight"] = kern.astype(np.float32)
        out[p + ".rbr_reparam.bias"] = bias.astype(np.float32)
    for name in ("seg.weight", "seg.bias"):
        out[name] = get(name).astype(np.float32)
    return out


def repvgg_dense_blocks(spec: ModelSpec, deploy_state_dict) -> tuple:
    """The RepSPK blocks (prefixes) of a deploy-form state_dict whose rbr_reparam.weight is non-zero at any
    of the eight dead taps: the library runs those on the dense 25-tap path, whatever `rsbb_taps` says
    (a hand-edited or fine-tuned deploy checkpoint; the converter's output has none)."""
    import numpy as np
    if repvgg_kernel_size(spec) != 5:
        return ()
    dead = []
    for p, *_ in repvgg_blocks(spec):
        w = deploy_state_dict[p + ".rbr_reparam.weight"]
        if hasattr(w, "detach"):
            w = w.detach().cpu().numpy()
        w = np.asarray(w)
        if any(np.any(w[:, :, kf, kt] != 0) for kf, kt in RSBB_DEAD_TAPS):
            dead.append(p)
    return tuple(dead)


def gemini_params(spec: ModelSpec) -> ParamList:
    """state_dict layout of Gemini_DF_ResNet (gemini_dfresnet.py:51-103): every downsample layer (0 is
    the stem) first, then the inverted bottlenecks stage by stage, then seg_1."""
    dims = GEMINI_DIMS
    out: ParamList = [("downsample_layers.0.0.weight", (dims[0], 1, 3, 3))] + _bn("downsample_layers.0.1", dims[0])
    for i in range(1, 5):
        out += [(f"downsample_layers.{i}.0.weight", (dims[i], dims[i - 1], 3, 3))] + _bn(f"downsample_layers.{i}.1", dims[i])
    for li, n in enumerate(GEMINI_ARCHS[spec.arch]):
        d = dims[li + 1]
        for bi in range(n):
            p = f"stages.{li}.{bi}"
            out += [(p + ".conv1.weight", (4 * d, d, 1, 1))] + _bn(p + ".bn1", 4 * d)
            out += [(p + ".conv2.weight", (4 * d, 1, 3, 3))] + _bn(p + ".bn2", 4 * d)
            out += [(p + ".conv3.weight", (d, 4 * d, 1, 1))] + _bn(p + ".bn3", d)
    stats_dim = int(spec.feat_dim / 16) * dims[4]
    out += [("seg_1.weight", (spec.embed_dim, stats_dim * 2)), ("seg_1.bias", (spec.embed_dim,))]
    if spec.two_emb_layer:
        out += [("seg_bn_1.running_mean", (spec.embed_dim,)), ("seg_bn_1.running_var", (spec.embed_dim,)),
                ("seg_bn_1.num_batches_tracked", ()),
                ("seg_2.weight", (spec.embed_dim, spec.embed_dim)), ("seg_2.bias", (spec.embed_dim,))]
    return out


def redimnet_stage_dims(arch: str):
    """Per stage (c_in, F_in, stride, c, F, blocks, hC): the 2-D view going in, after the entry conv,
    and the 1-D block's hidden width."""
    C, _, stages = REDIMNET_ARCHS[arch]
    c, F, out = C, REDIMNET_FEAT, []
    for s, n, red in stages:
        out.append((c, F, s, c * s, F // s, n, C * REDIMNET_FEAT // red))
        c, F = c * s, F // s
    return out


def redimnet_params(spec: ModelSpec) -> ParamList:
    """state_dict layout of ReDimNetB2 (redimnet.py:622-871): the input weights of the six stages and
    of the output, the stem, per stage the entry conv, its 2-D ConvNeXt blocks and the 1-D block
    (reduction + LayerNorm, four depthwise ConvNeXt blocks, the transformer layer, expansion), then
    the ASTP pooling (global context) and seg_1 (+ seg_bn_1 / seg_2)."""
    C, gd, stages = REDIMNET_ARCHS[spec.arch]
    D = C * spec.feat_dim
    out: ParamList = [("backbone.inputs_weights.0", (1, 1, 1, 1))]
    out += [(f"backbone.inputs_weights.{i}", (1, i + 1, D, 1)) for i in range(1, len(stages) + 1)]
    out += [("backbone.stem.0.weight", (C, 1, 3, 3)), ("backbone.stem.0.bias", (C,)),
            ("backbone.stem.1.weight", (C,)), ("backbone.stem.1.bias", (C,))]
    for si, (ci, _, s, c, _, n, hC) in enumerate(redimnet_stage_dims(spec.arch)):
        p = f"backbone.stage{si}"
        out += [(f"{p}.0.weight", (c, ci, s, 1)), (f"{p}.0.bias", (c,))]
        for bi in range(1, n + 1):
            q = f"{p}.{bi}.conv_block"
            out += [(q + ".dwconvs.0.weight", (c, gd, 3, 3)), (q + ".dwconvs.0.bias", (c,))] + _bn(q + ".norm", c)
            out += [(q + ".pwconv1.weight", (c, c, 1, 1)), (q + ".pwconv1.bias", (c,))]
        q = f"{p}.{n + 2}"  # index n + 1 is to1d, which has no parameters
        out += [(q + ".red_dim_conv.0.weight", (hC, D, 1)), (q + ".red_dim_conv.0.bias", (hC,)),
                (q + ".red_dim_conv.1.weight", (hC,)), (q + ".red_dim_conv.1.bias", (hC,))]
        for j, k in enumerate(REDIMNET_DW_KERNELS):
            r = f"{q}.tcm.{j}"
            out += [(r + ".dwconvs.0.weight", (hC, 1, k)), (r + ".dwconvs.0.bias", (hC,))] + _bn(r + ".norm", hC)
            out += [(r + ".pwconv1.weight", (hC, hC, 1)), (r + ".pwconv1.bias", (hC,))]
        r = f"{q}.tcm.4"
        for proj in ("k_proj", "v_proj", "q_proj", "out_proj"):
            out += [(f"{r}.attention.{proj}.weight", (hC, hC)), (f"{r}.attention.{proj}.bias", (hC,))]
        out += [(r + ".layer_norm.weight", (hC,)), (r + ".layer_norm.bias", (hC,))]
        for lin in ("intermediate_dense", "output_dense"):
            out += [(f"{r}.feed_forward.{lin}.weight", (hC, hC)), (f"{r}.feed_forward.{lin}.bias", (hC,))]
        out += [(r + ".final_layer_norm.weight", (hC,)), (r + ".final_layer_norm.bias", (hC,))]
        out += [(q + ".exp_dim_conv.weight", (D, hC, 1)), (q + ".exp_dim_conv.bias", (D,))]
    out += [("pool.linear1.weight", (128, 3 * D, 1)), ("pool.linear1.bias", (128,)),
            ("pool.linear2.weight", (D, 128, 1)), ("pool.linear2.bias", (D,))]
    out += [("seg_1.weight", (spec.embed_dim, 2 * D)), ("seg_1.bias", (spec.embed_dim,))]
    if spec.two_emb_layer:
        out += [("seg_bn_1.running_mean", (spec.embed_dim,)), ("seg_bn_1.running_var", (spec.embed_dim,)),
                ("seg_bn_1.num_batches_tracked", ()),
                ("seg_2.weight", (spec.embed_dim, spec.embed_dim)), ("seg_2.bias", (spec.embed_dim,))]
    return out


def param_list(spec: ModelSpec) -> ParamList:
    if spec.family == "res2net":
        return res2net_params(spec)
    if spec.family == "repvgg":
        return repvgg_params(spec)
    if spec.family == "redimnet":
        return redimnet_params(spec)
    if spec.family == "xvec":
        return xvec_params(spec)
    if spec.family == "gemini":
        return gemini_params(spec)
    if spec.family == "campplus":
        return campplus_params(spec)
    if spec.family == "eres2net":
        return eres2net_params(spec)
    if spec.family == "ecapa":
        return ecapa_params(spec)
    if spec.family == "simam":
        return simam_params(spec)
    return resnet_params(spec)


def xvec_gflop_per_utt(spec: ModelSpec, T: int) -> float:
    """Algorithmic FLOPs (2 x MACs) of one XVEC forward over T frames: every TDNN layer at the
    frames it keeps, XI's two 1x1 convs, seg_1 and seg_2."""
    macs, t, cin = 0, T, spec.feat_dim
    for i, (k, d) in enumerate(XVEC_FRAMES, 1):
        t -= (k - 1) * d
        cout = XVEC_STATS if i == 5 else XVEC_HID
        macs += t * cout * cin * k
        cin = cout
    xi = spec.pooling_func == "XI"
    if xi:
        macs += t * 2 * XVEC_STATS * XI_HIDDEN
    macs += XVEC_STATS * (1 if xi else 2) * spec.embed_dim + spec.embed_dim ** 2
    return 2.0 * macs / 1e9


def simam_gflop_per_utt(spec: ModelSpec, T: int) -> float:
    """Algorithmic FLOPs (2 x MACs) of one SimAM-ResNet forward over T frames."""
    m, F, t = spec.m_channels, spec.feat_dim, T
    macs = F * t * m * 9  # stem
    cin = m
    for li, n in enumerate(SIMAM_ARCHS[spec.arch]):
        planes = m * (2 ** li)
        for bi in range(n):
            stride = 2 if (li > 0 and bi == 0) else 1
            Fo, To = (F - 1) // stride + 1, (t - 1) // stride + 1
            macs += Fo * To * planes * (cin * 9 + planes * 9)
            if stride != 1 or cin != planes:
                macs += Fo * To * planes * cin
            F, t, cin = Fo, To, planes
    cf = cin * F
    macs += t * (cf * 128 * 2) + 2 * cf * spec.embed_dim
    return 2.0 * macs / 1e9


def campplus_gflop_per_utt(spec: ModelSpec, T: int) -> float:
    """Algorithmic FLOPs (2 x MACs) of one CAMPPlus forward over T frames: FCM head, strided TDNN,
    the dense layers (1x1 conv, k3 local conv, mask linears per segment), transits, embedding."""
    layers, _ = CAMPP_ARCHS[spec.arch]
    F = spec.feat_dim
    macs = F * T * 32 * 9  # stem
    for _ in (1, 2):
        F //= 2
        macs += F * T * 32 * (288 + 32 + 288)  # strided block: conv1, shortcut, conv2
        macs += F * T * 32 * (288 + 288)       # plain block
    F //= 2
    macs += F * T * 32 * 288                   # head.conv2
    t = (T - 1) // 2 + 1
    nseg = (t + CAMPP_SEG - 1) // CAMPP_SEG
    macs += t * 128 * 32 * F * 5               # xvector.tdnn
    ch = 128
    for n in layers:
        for i in range(n):
            macs += t * 128 * (ch + 32 * i) + t * 32 * 384 + nseg * (128 * 64 + 64 * 32)
        ch += 32 * n
        macs += t * ch * (ch // 2)
        ch //= 2
    macs += 2 * ch * spec.embed_dim
    return 2.0 * macs / 1e9


def eres2net_gflop_per_utt(spec: ModelSpec, T: int) -> float:
    """Algorithmic FLOPs (2 x MACs) of one ERes2Net forward over T frames: stem, every block's 1x1 and
    3x3 convs, its AFFs (2C -> C/4 -> C), shortcuts, the bottom-up downsample convs and AFFs, seg_1."""
    m, _, scale, exp = ERES2NET_ARCHS[spec.arch]
    F, t = spec.feat_dim, T
    macs = F * t * m * 9
    pos = {}
    for p, in_planes, planes, w, stride, aff, has_sc in eres2net_blocks(spec):
        F, t = (F - 1) // stride + 1, (t - 1) // stride + 1
        n = F * t
        macs += n * (in_planes * w * scale + scale * 9 * w * w + w * scale * planes * exp)
        if aff:
            macs += n * (scale - 1) * (2 * w * (w // 4) + (w // 4) * w)
        if has_sc:
            macs += n * in_planes * planes * exp
        pos[p.split(".")[0]] = n
    c = m * exp
    for i in (1, 2, 3):
        ci, co, n = c * 2 ** (i - 1), c * 2 ** i, pos[f"layer{i + 1}"]
        macs += n * (9 * ci * co + 2 * co * (co // 4) + (co // 4) * co)
    macs += 2 * c * 8 * F * spec.embed_dim + (spec.embed_dim ** 2 if spec.two_emb_layer else 0)
    return 2.0 * macs / 1e9


def res2net_gflop_per_utt(spec: ModelSpec, T: int) -> float:
    """Algorithmic FLOPs (2 x MACs) of one Res2Net forward over T frames: stem, every block's conv1,
    3x3 conv, conv3 and projection shortcut, seg_1 (+ seg_2)."""
    m, exp = RES2NET_ARCHS[spec.arch], RES2NET_EXPANSION
    F, t = spec.feat_dim, T
    macs = F * t * m * 9
    for p, in_planes, planes, w, stride, has_sc in res2net_blocks(spec):
        F, t = (F - 1) // stride + 1, (t - 1) // stride + 1
        macs += F * t * (in_planes * 2 * w + 9 * w * w + 2 * w * planes * exp)
        if has_sc:
            macs += F * t * in_planes * planes * exp
    macs += 2 * m * exp * 8 * F * spec.embed_dim + (spec.embed_dim ** 2 if spec.two_emb_layer else 0)
    return 2.0 * macs / 1e9


def repvgg_gflop_per_utt(spec: ModelSpec, T: int, rsbb_taps: int = 1, dense_blocks=()) -> float:
    """FLOPs (2 x MACs) one RepVGG forward over T frames executes: every block as its one folded conv
    (9 taps; a RepSPK block 17 taps on the sparse path, rsbb_taps = 1, and 25 on the dense path,
    rsbb_taps = 0 or a block named in `dense_blocks`, see repvgg_dense_blocks), then seg.  The dense figure of
    a RepSPK model, repvgg_gflop_per_utt(spec, T, 0), is 25 / 17 of the sparse one in the convs.  Channel
    padding (widths 48 and 96 run as 64 and 128) is not counted."""
    k = repvgg_kernel_size(spec)
    F, t, macs, cout = spec.feat_dim, T, 0, 0
    for p, _, cin, cout, stride, _ in repvgg_blocks(spec):
        F, t = (F - 1) // stride + 1, (t - 1) // stride + 1
        taps = 9 if k == 3 else (17 if rsbb_taps and p not in dense_blocks else 25)
        macs += F * t * cout * cin * taps
    macs += 2 * cout * F * spec.embed_dim
    return 2.0 * macs / 1e9


def gemini_gflop_per_utt(spec: ModelSpec, T: int) -> float:
    """Algorithmic FLOPs (2 x MACs) of one Gemini DF-ResNet forward over T frames, convolutions only:
    the stem, per level the downsample conv and its inverted bottlenecks (two 1x1 convs of 4 d^2 and
    the depthwise 3x3 of 36 d MACs per position), seg_1."""
    dims = GEMINI_DIMS
    F, t = spec.feat_dim, T
    macs = F * t * dims[0] * 9
    for li, n in enumerate(GEMINI_ARCHS[spec.arch]):
        F, t = (F - 1) // 2 + 1, (t - 1) // GEMINI_STRIDE_T[li] + 1
        d = dims[li + 1]
        macs += F * t * (9 * dims[li] * d + n * (8 * d * d + 36 * d))
    macs += 2 * F * dims[4] * spec.embed_dim
    return 2.0 * macs / 1e9


def redimnet_gflop_per_utt(spec: ModelSpec, T: int) -> float:
    """Algorithmic FLOPs (2 x MACs) of one ReDimNetB2 forward over T frames: the stem, per stage the
    entry conv, the 2-D blocks (grouped 3x3 + 1x1), the 1-D block (reduction, four depthwise + 1x1
    blocks, the six hC x hC linears, attention's two T x T products, expansion), pool.linear1 / 2
    and seg_1 (+ seg_2)."""
    C, gd, _ = REDIMNET_ARCHS[spec.arch]
    D = C * spec.feat_dim
    macs = T * D * 9
    for ci, _, s, c, _, n, hC in redimnet_stage_dims(spec.arch):
        macs += T * D * (s * ci + n * (9 * gd + c))
        macs += T * (2 * D * hC + sum(REDIMNET_DW_KERNELS) * hC + 4 * hC * hC + 6 * hC * hC) + 2 * T * T * hC
    macs += T * 2 * D * 128 + 2 * D * 128 + 2 * D * spec.embed_dim + (spec.embed_dim ** 2 if spec.two_emb_layer else 0)
    return 2.0 * macs / 1e9


def resnet_gflop_per_utt(spec: ModelSpec, T: int) -> float:
    """Algorithmic FLOPs (2 x MACs) of one ResNet forward over T frames (resnet.py:35-204):
    stem, every block's convs (+ projection shortcuts), the pooled-statistics embedding."""
    kind, nblocks = RESNET_ARCHS[spec.arch]
    m, F, t = spec.m_channels, spec.feat_dim, T
    exp = 1 if kind == "basic" else 4
    macs = F * t * m * 9  # stem 3x3, 1 -> m
    cin = m
    for li, n in enumerate(nblocks):
        p = m * (2 ** li)
        for bi in range(n):
            s = 2 if (li > 0 and bi == 0) else 1
            Fo, To = (F - 1) // s + 1, (t - 1) // s + 1
            if kind == "basic":
                macs += Fo * To * p * (cin * 9 + p * 9)
            else:
                macs += F * t * cin * p + Fo * To * (p * p * 9 + p * 4 * p)
            if s != 1 or cin != exp * p:
                macs += Fo * To * cin * exp * p
            F, t, cin = Fo, To, exp * p
    macs += 2 * cin * F * spec.embed_dim + (spec.embed_dim ** 2 if spec.two_emb_layer else 0)
    return 2.0 * macs / 1e9


def ecapa_gflop_per_utt(spec: ModelSpec, T: int) -> float:
    """Algorithmic FLOPs (2 x MACs) of one ECAPA forward over T frames."""
    xi = spec.arch in XI_ECAPA_ARCHS
    C, glob = (XI_ECAPA_ARCHS[spec.arch], False) if xi else ECAPA_ARCHS[spec.arch]
    w = C // 8
    if xi:  # the trunk, XI's lin1 / lin2 (1536 <-> 256), the 1536-wide head
        return 2.0 * (spec.feat_dim * 5 * C * T + 3 * (2 * C * C * T + 7 * w * w * 3 * T + 2 * C * 128)
                      + 3 * C * 1536 * T + 2 * 1536 * XI_HIDDEN * T + 1536 * spec.embed_dim) / 1e9
    macs = spec.feat_dim * 5 * C * T                       # layer1
    macs += 3 * (2 * C * C * T + 7 * w * w * 3 * T + 2 * C * 128)  # blocks
    macs += 3 * C * 1536 * T                                # conv
    # pool.linear1: GLOB's mean/std context columns are constant over T and
    # are folded into a per-utterance bias, so both variants run
    # a 1536-deep contraction per frame.
    macs += 1536 * 128 * T + (2 * 1536 * 128 if glob else 0)
    macs += 128 * 1536 * T                                  # pool.linear2
    macs += 3072 * spec.embed_dim
    return 2.0 * macs / 1e9


# ---------------------------------------------------------------- HuBERT ---
# s3prl HuBERT-base upstream as wrapped by wespeaker/frontend/s3prl.py:23-93.
# Canonical keys are the fairseq names s3prl loads, under the prefix the
# reference checkpoint uses (`model.add_module("frontend", ...)`,
# bin/extract.py:49-55 -> S3PRLUpstream.upstream.model).
HUBERT_PREFIX = "frontend.upstream.upstream.model."
HUBERT_BASE = dict(conv_dim=512, conv_kernel=(10, 3, 3, 3, 3, 2, 2), conv_stride=(5, 2, 2, 2, 2, 2, 2),
                   hidden=768, layers=12, heads=12, ffn=3072, pos_k=128, pos_groups=16)


def hubert_params(cfg=HUBERT_BASE, prefix: str = HUBERT_PREFIX) -> ParamList:
    c, h = cfg["conv_dim"], cfg["hidden"]
    out: ParamList = []
    for i, k in enumerate(cfg["conv_kernel"]):
        out.append((f"feature_extractor.conv_layers.{i}.0.weight", (c, 1 if i == 0 else c, k)))
        if i == 0:
            out += [("feature_extractor.conv_layers.0.2.weight", (c,)),
                    ("feature_extractor.conv_layers.0.2.bias", (c,))]
    out += [("layer_norm.weight", (c,)), ("layer_norm.bias", (c,)),
            ("post_extract_proj.weight", (h, c)), ("post_extract_proj.bias", (h,)),
            ("encoder.pos_conv.0.bias", (h,)), ("encoder.pos_conv.0.weight_g", (1, 1, cfg["pos_k"])),
            ("encoder.pos_conv.0.weight_v", (h, h // cfg["pos_groups"], cfg["pos_k"])),
            ("encoder.layer_norm.weight", (h,)), ("encoder.layer_norm.bias", (h,))]
    for li in range(cfg["layers"]):
        p = f"encoder.layers.{li}."
        for proj in ("k_proj", "v_proj", "q_proj", "out_proj"):
            out += [(p + f"self_attn.{proj}.weight", (h, h)), (p + f"self_attn.{proj}.bias", (h,))]
        out += [(p + "self_attn_layer_norm.weight", (h,)), (p + "self_attn_layer_norm.bias", (h,)),
                (p + "fc1.weight", (cfg["ffn"], h)), (p + "fc1.bias", (cfg["ffn"],)),
                (p + "fc2.weight", (h, cfg["ffn"])), (p + "fc2.bias", (h,)),
                (p + "final_layer_norm.weight", (h,)), (p + "final_layer_norm.bias", (h,))]
    out = [(prefix + n, s) for n, s in out]
    out.append(("frontend.featurizer.weights", (cfg["layers"] + 1,)))
    return out


def hubert_num_frames(num_samples: int, cfg=HUBERT_BASE) -> int:
    t = num_samples
    for k, s in zip(cfg["conv_kernel"], cfg["conv_stride"]):
        t = (t - k) // s + 1
    return t


def s3prl_num_frames(num_samples: int, downsample_rate: int = 320) -> int:
    """len(range(0, W, 320)) — s3prl's length match target."""
    return (num_samples + downsample_rate - 1) // downsample_rate


def hubert_gflop_per_utt(num_samples: int, cfg=HUBERT_BASE) -> float:
    """Algorithmic FLOPs (2 x MACs) of the HuBERT-base front end on one utterance."""
    c, h, L = cfg["conv_dim"], cfg["hidden"], cfg["layers"]
    t = num_samples
    macs = 0
    for i, (k, s) in enumerate(zip(cfg["conv_kernel"], cfg["conv_stride"])):
        t = (t - k) // s + 1
        macs += t * c * k * (1 if i == 0 else c)
    macs += t * c * h                                               # post_extract_proj
    macs += t * h * (h // cfg["pos_groups"]) * cfg["pos_k"]         # grouped pos_conv
    per_layer = t * h * 3 * h + 2 * t * t * h + t * h * h + 2 * t * h * cfg["ffn"]
    return 2.0 * (macs + L * per_layer) / 1e9


# ----------------------------------------------------------------- WavLM ---
# s3prl `wavlm_base` / `wavlm_base_plus`: HuBERT-base in every shape, plus a gated, bucketed
# relative-position bias on every attention score (published WavLM source; transformers' WavLMModel
# is the offline proxy).  Layer 0 owns the bucket embedding, every layer its own gate.
WAVLM_BASE = dict(HUBERT_BASE, rel_buckets=320, rel_max_distance=800, gate_dim=8)
WAVLM_UPSTREAMS = ("wavlm_base", "wavlm_base_plus")


def wavlm_params(cfg=WAVLM_BASE, prefix: str = HUBERT_PREFIX) -> ParamList:
    """hubert_params() with, behind each layer's final_layer_norm, the layer's gate
    (grep_linear, grep_a) and, in layer 0, relative_attention_bias.weight (buckets, heads)."""
    H = cfg["heads"]
    dh = cfg["hidden"] // H
    out: ParamList = []
    for name, shape in hubert_params(cfg, prefix):
        out.append((name, shape))
        if name.endswith(".final_layer_norm.bias"):
            p = name[:-len("final_layer_norm.bias")] + "self_attn."
            if ".layers.0." in name:
                out.append((p + "relative_attention_bias.weight", (cfg["rel_buckets"], H)))
            out += [(p + "grep_linear.weight", (cfg["gate_dim"], dh)), (p + "grep_linear.bias", (cfg["gate_dim"],)),
                    (p + "grep_a", (1, H, 1, 1))]
    return out


def wavlm_rel_bucket(d: int, cfg=WAVLM_BASE) -> int:
    """Bucket of the relative position d = key - query (bidirectional: d > 0, the key after
    the query, takes the upper half).  Constant for |d| >= 778."""
    import math
    n = cfg["rel_buckets"] // 2
    exact = n // 2
    r = abs(d)
    b = n if d > 0 else 0
    if r < exact:
        return b + r
    return b + min(n - 1, int(exact + math.log(r / exact) / math.log(cfg["rel_max_distance"] / exact) * (n - exact)))


def wavlm_gflop_per_utt(num_samples: int, cfg=WAVLM_BASE) -> float:
    """hubert_gflop_per_utt plus the gate (two 64-long dot products per frame and head) and one
    multiply-add per attention score."""
    t = hubert_num_frames(num_samples, cfg)
    extra = cfg["layers"] * (2 * t * cfg["hidden"] + t * t * cfg["heads"])
    return hubert_gflop_per_utt(num_samples, cfg) + 2.0 * extra / 1e9
