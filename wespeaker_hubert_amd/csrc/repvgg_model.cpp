// RepVGG (repvgg.py:456-747) in deploy form: parameter table, packing, workspace and the forward schedule.
// The library knows the re-parameterised layout only: every block is rbr_reparam.{weight [cout][cin][k][k],
// bias} (k = 3 for a RepVGG block, 5 for a RepSPK block of the *_RSBB_* names), then seg.  A training-form
// checkpoint is folded on the host before it gets here (arch.repvgg_fold in the Python package).
// NHWC activations [B][F][T][C]; a block is one conv + bias + ReLU, so the trunk is a plain chain:
//   stage0    launch_resnet_stem (3x3, C0 = 32 / 64) or launch_repvgg_stem (17 taps, or C0 = 48)
//   RepVGG    conv3x3_img for stride-1 blocks of 32 / 64 / 128 channels, else the 2-D implicit GEMM
//   RepSPK    launch_rsbb_conv over the 17 live taps (repvgg.hip), or the dense 25-tap 2-D implicit GEMM
//             (option rsbb_taps; always for a block whose loaded weight is non-zero at a dead tap)
//   TSTP over the (c, f) rows (launch_frame_stats) and seg (the small linear), as the ResNets'
// Widths 48 and 96 (A0, A2) do not meet the kernels' cin % 32 / N % 64 rules: their channels are padded to
// 64 and 128 with zero weights and zero bias at pack time, and ReLU keeps the padding at 0.  The cost is
// the padded share of the MACs and of the activation traffic: (64 / 48)^2 = 1.78x the MACs of a 48 -> 48
// block (A0 stage 1: 2 blocks) and (128 / 96)^2 = 1.78x of a 96 -> 96 block (A0 stage 2, A2 stage 1).
#include "conv3x3_img.h"
#include "model_impl.h"
#include "repvgg.h"

namespace wsp {

namespace {
struct Arch {
  const char* name;
  bool spk;  // RepSPK blocks
  int nblocks[4];
  int c0, widths[4];
  bool sparse[5];  // rsbb_taps = 1: the stages (0 = the stem) that run the 17-tap kernel (DESIGN.md has the table)
};
const Arch kArchs[] = {
    {"REPVGG_TINY_A0", false, {3, 4, 23, 3}, 32, {32, 64, 128, 256}, {}},
    {"REPVGG_TINY_RSBB_A0", true, {3, 4, 23, 3}, 32, {32, 64, 128, 256}, {true, true, true, true, true}},
    {"REPVGG_A0", false, {2, 4, 14, 1}, 48, {48, 96, 192, 1280}, {}},
    {"REPVGG_RSBB_A0", true, {2, 4, 14, 1}, 48, {48, 96, 192, 1280}, {true, true, true, true, true}},
    {"REPVGG_A1", false, {2, 4, 14, 1}, 64, {64, 128, 256, 1280}, {}},
    {"REPVGG_A2", false, {2, 4, 14, 1}, 64, {96, 192, 384, 1408}, {}},
    {"REPVGG_RSBB_A2", true, {2, 4, 14, 1}, 64, {96, 192, 384, 1408}, {true, true, true, true, true}},
    {"REPVGG_B0", false, {4, 6, 16, 1}, 64, {64, 128, 256, 1280}, {}},
    {"REPVGG_RSBB_B0", true, {4, 6, 16, 1}, 64, {64, 128, 256, 1280}, {true, true, true, true, true}},
};
// the constructors of repvgg.py the path refuses by name
const char* const kOthers[] = {"REPVGG_B1",   "REPVGG_B2",   "REPVGG_B3",   "REPVGG_B1g2", "REPVGG_B1g4",
                               "REPVGG_B2g2", "REPVGG_B2g4", "REPVGG_B3g2", "REPVGG_B3g4", "REPVGG_D2SE"};

int padded(int c) { return c == 32 ? 32 : round_up(c, 64); }  // 48 -> 64, 96 -> 128; the other widths stay

struct RepVgg final : Model::Impl {
  using Impl::Impl;
  const Arch* a = nullptr;
  struct Block {
    std::string name;
    int stage = 0, cin = 0, cout = 0, stride = 1;
    int cinp = 0, coutp = 0;  // padded widths
    ConvW dense;              // all k x k taps (the 2-D implicit GEMM; .frag: conv3x3_img)
    ConvW live;               // RepSPK: the 17 live taps (launch_rsbb_conv); .whi null: a dead tap is non-zero
  };
  std::vector<Block> blocks;   // blocks[0] = stage0
  float *stem_w = nullptr, *stem_b = nullptr;
  int stem_taps = 9;  // 9; RepSPK: 17, or 25 when a dead tap of stage0 is non-zero
  LinW seg;
  struct Ws {
    float *X, *O, *pooled, *scratch;
    size_t scratch_floats, floats;
    int bc;  // utterances per forward chunk, by the widest activation operand of any block
  };

  void build_params() override;
  void finalize() override;
  bool owns_option(const std::string& key) const override { return key == "rsbb_taps"; }
  void check_forward(int B, int T) const override;
  Ws ws_layout(int B, int T, float* base) const;
  size_t ws_floats(int B, int T) const override { return ws_layout(B, T, nullptr).floats; }
  bool sparse(const Block& b) const {
    return a->spk && b.live.whi && (opt.rsbb_taps == 2 || (opt.rsbb_taps == 1 && a->sparse[b.stage]));
  }
  void gemm2d(const char* tag, const ConvW& cw, const float* x, int ldx, float* out, int B, int Fi, int Ti, int kw,
              int stride, hipStream_t s);
  void forward(const float* feats, int B, int T, float* embed, float* ws, hipStream_t s) override;
};
}  // namespace

Model::Impl* make_repvgg(const std::string& arch, int feat_dim, int embed_dim, bool emb_bn, bool two_emb) {
  for (const char* o : kOthers)
    WSP_CHECK(arch != o, "unsupported arch " + arch +
                             ": the RepVGG path implements TINY_A0 / A0 / A1 / A2 / B0 and their RSBB variants (no "
                             "grouped convs, no SE block, stage-4 widths up to 1408)");
  const Arch* a = std::find_if(std::begin(kArchs), std::end(kArchs), [&](const Arch& k) { return arch == k.name; });
  if (a == std::end(kArchs)) return nullptr;
  WSP_CHECK(!emb_bn && !two_emb, "RepVGG has no emb_bn / two_emb_layer");
  // repvgg.py:520 sizes the pooling for int(feat_dim / 8) frequency rows while stage 4 keeps ceil(feat_dim / 8)
  WSP_CHECK(feat_dim >= 8 && feat_dim % 8 == 0, "RepVGG feat_dim must be a positive multiple of 8");
  WSP_CHECK(embed_dim > 0, "embed_dim must be positive");
  RepVgg* m = new RepVgg(arch, feat_dim, embed_dim, emb_bn, two_emb);
  m->a = a;
  m->opt.x3_variant = 4;  // 256 x 128 swizzled, as the basic-block ResNets (MFMA-bound 3x3 / 5x5 convs)
  return m;
}

// deploy-form state_dict order (convert_model.pt): 70 entries for the TINY models, 46 for A0 / A1 / A2, 58 for B0
void RepVgg::build_params() {
  const int k = a->spk ? 5 : 3;
  auto block = [&](const std::string& name, int stage, int cin, int cout, int stride) {
    Block b;
    b.name = name;
    b.stage = stage;
    b.cin = cin;
    b.cout = cout;
    b.stride = stride;
    b.cinp = cin == 1 ? 1 : padded(cin);
    b.coutp = padded(cout);
    add(name + ".rbr_reparam.weight", {cout, cin, k, k});
    add(name + ".rbr_reparam.bias", {cout});
    blocks.push_back(b);
  };
  block("stage0", 0, 1, a->c0, 1);
  int cin = a->c0;
  for (int li = 0; li < 4; ++li)
    for (int bi = 0; bi < a->nblocks[li]; ++bi) {
      block("stage" + std::to_string(li + 1) + "." + std::to_string(bi), li + 1, cin, a->widths[li],
            (li > 0 && bi == 0) ? 2 : 1);
      cin = a->widths[li];
    }
  add("seg.weight", {embed_dim, 2 * cin * (feat_dim / 8)});
  add("seg.bias", {embed_dim});
}

void RepVgg::finalize() {
  const int k = a->spk ? 5 : 3, kk = k * k;
  auto dead = [&](int tap) {  // of a 5x5 kernel: not among the live taps
    for (int j = 0; j < kRsbbLiveTaps; ++j)
      if (kRsbbTaps[j][0] * 5 + kRsbbTaps[j][1] == tap) return false;
    return true;
  };
  for (Block& b : blocks) {
    const std::vector<float>& W = P(b.name + ".rbr_reparam.weight");
    const std::vector<float>& bias = P(b.name + ".rbr_reparam.bias");
    bool dead_zero = true;
    if (a->spk)
      for (size_t i = 0; i < W.size() && dead_zero; ++i)
        if (W[i] != 0.f && dead((int)(i % 25))) dead_zero = false;
    if (b.stage == 0) {
      // the stem kernels take [C0][taps]: 3x3 or 5x5 row-major, or the 17 live taps.  The stem is f32 FMAs, not
      // a GEMM: a RepSPK stem runs its 17 live taps whatever rsbb_taps says, and all 25 if a dead tap is non-zero
      stem_taps = !a->spk ? 9 : dead_zero ? kRsbbLiveTaps : 25;
      std::vector<float> w;
      if (stem_taps == kRsbbLiveTaps) {
        w.resize((size_t)b.cout * kRsbbLiveTaps);
        for (int n = 0; n < b.cout; ++n)
          for (int j = 0; j < kRsbbLiveTaps; ++j)
            w[(size_t)n * kRsbbLiveTaps + j] = W[(size_t)n * 25 + kRsbbTaps[j][0] * 5 + kRsbbTaps[j][1]];
      } else {
        w = W;
      }
      stem_w = dev.upload(w);
      stem_b = dev.upload(bias);
      continue;
    }
    // zero-padded channels: [coutp][cinp][k*k]
    std::vector<float> wp((size_t)b.coutp * b.cinp * kk, 0.f), bp(b.coutp, 0.f);
    for (int n = 0; n < b.cout; ++n) {
      bp[n] = bias[n];
      for (int c = 0; c < b.cin; ++c)
        std::copy(&W[((size_t)n * b.cin + c) * kk], &W[((size_t)n * b.cin + c) * kk] + kk,
                  &wp[((size_t)n * b.cinp + c) * kk]);
    }
    b.dense = pack_conv(wp, b.coutp, b.cinp, kk, bp.data(), "");
    // conv3x3_img.hip: fragments in the same k = tap * cin + c order as the implicit GEMM's packed image
    if (kk == 9 && b.stride == 1 && b.coutp == b.cinp && conv3x3_img_supported(b.cinp))
      b.dense.frag = pack_frag(pack::conv_kmajor(wp, b.coutp, b.cinp, 9, 9 * b.cinp), b.coutp, 9 * b.cinp);
    if (a->spk && dead_zero) {
      std::vector<float> wl((size_t)b.coutp * b.cinp * kRsbbLiveTaps);
      for (size_t nc = 0; nc < (size_t)b.coutp * b.cinp; ++nc)
        for (int j = 0; j < kRsbbLiveTaps; ++j)
          wl[nc * kRsbbLiveTaps + j] = wp[nc * 25 + kRsbbTaps[j][0] * 5 + kRsbbTaps[j][1]];
      b.live = pack_conv(wl, b.coutp, b.cinp, kRsbbLiveTaps, bp.data(), "");  // k = j * cinp + c (repvgg.h)
    }
  }
  // seg over TSTP stats; reference flatten index s*C*F4 + c*F4 + f, ours f*2C + s*C + c (C4 is never padded)
  const int C4 = blocks.back().cout, F4 = feat_dim / 8;
  WSP_CHECK(blocks.back().coutp == C4, "RepVGG: the last stage's width must not need padding");
  const auto& W = P("seg.weight");
  const int K = 2 * C4 * F4;
  std::vector<float> wp((size_t)embed_dim * K);
  for (int n = 0; n < embed_dim; ++n)
    for (int f = 0; f < F4; ++f)
      for (int sidx = 0; sidx < 2; ++sidx)
        for (int c = 0; c < C4; ++c)
          wp[(size_t)n * K + f * 2 * C4 + sidx * C4 + c] = W[(size_t)n * K + sidx * C4 * F4 + c * F4 + f];
  seg = pack_lin(wp.data(), embed_dim, K, K, P("seg.bias").data());
}

void RepVgg::check_forward(int, int T) const {
  // as every family off the f32 GEMM path: the message names the first of them
  WSP_CHECK(opt.precision == 1, "ResNet runs on the bf16x3 kernels only (precision=1)");
  // T' = 1 makes TSTP's unbiased variance NaN in the reference
  WSP_CHECK((T + 7) / 8 >= 2, "RepVGG needs >= 9 frames (2 after the three stride-2 stages)");
}

RepVgg::Ws RepVgg::ws_layout(int B, int T, float* base) const {
  size_t big = 0;  // floats per utterance of the widest activation
  int Fi = feat_dim, Ti = T;
  for (const Block& b : blocks) {
    Fi = (Fi - 1) / b.stride + 1;
    Ti = (Ti - 1) / b.stride + 1;
    big = std::max(big, (size_t)Fi * Ti * b.coutp);
  }
  const size_t K = (size_t)Fi * 2 * blocks.back().coutp;
  WsCursor c{base};
  Ws w;
  w.bc = chunk_for(B, big * sizeof(float));
  const size_t bc = w.bc;
  w.X = c.take(bc * big);
  w.O = c.take(bc * big);
  w.pooled = c.take(bc * K);
  w.scratch_floats = small_linear_scratch_floats((int)bc, embed_dim, (int)K);
  w.scratch = c.take(w.scratch_floats);
  w.floats = c.off;
  return w;
}

// cw over all kw x kw taps, pad kw / 2, + bias + ReLU on the 2-D implicit GEMM
void RepVgg::gemm2d(const char* tag, const ConvW& cw, const float* x, int ldx, float* out, int B, int Fi, int Ti, int kw,
                    int stride, hipStream_t s) {
  ConvGemmArgs g{};
  one_operand(g, x, ldx, cw.cin);
  const int pad = kw / 2;
  const int Fo = (Fi - 1) / stride + 1, To = (Ti - 1) / stride + 1;
  const int M = B * Fo * To;
  fill(g, cw, M, M, 1, pad, out, cw.N, kActRelu, nullptr, true, nullptr, 0);
  g.conv2d = 1;
  g.Fi = Fi;
  g.Ti = Ti;
  g.Fo = Fo;
  g.To = To;
  g.stride = stride;
  g.kw = kw;
  run(tag, 2.0 * M * cw.N * cw.K, s, [&] { launch_conv_gemm_x3(g, cw.whi, cw.wlo, opt.x3_variant, s); });
}

void RepVgg::forward(const float* feats, int B, int T, float* embed, float* ws, hipStream_t s) {
  const Ws W = ws_layout(B, T, ws);
  const int bc = W.bc;
  static const char* kImg[5] = {"", "rep_conv3x3.L1", "rep_conv3x3.L2", "rep_conv3x3.L3", "rep_conv3x3.L4"};
  static const char* kLive[5] = {"", "rsbb_sparse.L1", "rsbb_sparse.L2", "rsbb_sparse.L3", "rsbb_sparse.L4"};
  static const char* kDense[5] = {"", "rsbb_dense.L1", "rsbb_dense.L2", "rsbb_dense.L3", "rsbb_dense.L4"};
  for (int b0 = 0; b0 < B; b0 += bc) {
    const int nb = std::min(bc, B - b0);
    int Fi = feat_dim, Ti = T, Ci = blocks[0].coutp;
    const float* f0 = feats + (size_t)b0 * T * feat_dim;
    run("stem", 0, s, [&] {
      if (!a->spk && Ci == a->c0)
        launch_resnet_stem(f0, nb, T, feat_dim, a->c0, stem_w, stem_b, W.X, s);
      else
        launch_repvgg_stem({f0, nb, T, feat_dim, a->c0, Ci, stem_taps, stem_w, stem_b, W.X, Ci}, s);
    });
    float* x = W.X;
    float* o = W.O;
    for (size_t ib = 1; ib < blocks.size(); ++ib) {
      const Block& b = blocks[ib];
      const int Fo = (Fi - 1) / b.stride + 1, To = (Ti - 1) / b.stride + 1;
      if (sparse(b)) {
        const RsbbConvArgs r{x, Ci, nb, Fi, Ti, b.cinp, b.stride, b.live.whi, b.live.wlo, b.live.bias, b.coutp, o, b.coutp};
        run(kLive[b.stage], 2.0 * nb * Fo * To * b.coutp * b.live.K, s, [&] { launch_rsbb_conv(r, s); });
      } else if (a->spk) {
        gemm2d(kDense[b.stage], b.dense, x, Ci, o, nb, Fi, Ti, 5, b.stride, s);
      } else if (b.dense.frag && opt.conv3x3_img && (b.cinp <= 64 || opt.conv3x3_img >= 2)) {
        const Conv3x3Args c{x, o, nb, Fi, Ti, b.dense.frag, b.dense.bias, nullptr, nullptr, nullptr, 1, opt.conv3x3_img};
        run(kImg[b.stage], 2.0 * nb * Fi * Ti * b.coutp * b.dense.K, s, [&] { launch_conv3x3_img(c, b.coutp, s); });
      } else {
        gemm2d(kImg[b.stage], b.dense, x, Ci, o, nb, Fi, Ti, 3, b.stride, s);
      }
      std::swap(x, o);
      Fi = Fo;
      Ti = To;
      Ci = b.coutp;
    }
    // TSTP over frames for every (utterance, freq) row block, then seg
    run("tstp_head", 0, s, [&] {
      launch_frame_stats(x, Ci, nb * Fi, Ti, Ci, W.pooled, 2 * Ci, 1, Ci, s);
      launch_small_linear({W.pooled, Fi * 2 * Ci, seg.wt, seg.bias, embed + (size_t)b0 * embed_dim, embed_dim, nb,
                           Fi * 2 * Ci, embed_dim, 0, W.scratch_floats ? W.scratch : nullptr, W.scratch_floats},
                          s);
    });
  }
}

}  // namespace wsp
