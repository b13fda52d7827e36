// Gemini DF-ResNet (gemini_dfresnet.py:30-178): parameter table, BatchNorm folds / packing,
// workspace and the forward schedule.  NHWC activations [B][F][T][C].  The network is a stem (3x3,
// 1 -> 32, ReLU), then four levels of a 3x3 downsample conv (frequency stride 2, time stride 2 at
// level 2 only, BN, no activation) followed by depths[i] inverted bottlenecks of width d = dims[i]:
// conv1 (1x1, d -> 4d, ReLU), conv2 (depthwise 3x3, ReLU), conv3 (1x1, 4d -> d) + x, ReLU.  The four
// constructors differ only in the depths, which are data.  conv1 runs on the shared implicit GEMM
// (Impl::gemm, tile family 7: measured 1.74 ms against 3.17 ms on launch_eres_pw for Gemini114 at
// B = 64 x T = 200); option ib_fused picks the rest of a block: 0 = launch_gemini_dw, then conv3 with
// residual and ReLU on the same GEMM (1.77 ms against 3.00 ms); 1 = launch_gemini_tail (conv2 inside
// conv3's operand).  The stem and the TSTP head are the ResNet's.
#include "gemini.h"
#include "model_impl.h"

namespace wsp {

namespace {
constexpr int kDims[5] = {32, 32, 64, 128, 256};
constexpr int kStrideT[4] = {1, 2, 1, 1};  // the frequency stride is 2 at every level

struct Gemini final : Model::Impl {
  using Impl::Impl;
  int depths[4] = {3, 3, 9, 3};
  float *stem_w = nullptr, *stem_b = nullptr;
  struct Pw {  // BN-folded conv as pack::frag16 fragments + bias
    void* w = nullptr;
    float* b = nullptr;
    int N = 0, K = 0;
  };
  struct Block {
    std::string name;
    int d = 0;
    ConvW c1, c3g;  // the 1x1 convs on the shared GEMM, BN folded in (bias = the BN's shift)
    Pw c3;          // conv3 again as the tail kernel's fragments
    float *w2 = nullptr, *b2 = nullptr;  // depthwise taps [9][4d] with BN2 folded in, its shift [4d]
  };
  Pw down[4];
  std::vector<Block> blocks;
  LinW seg1, seg2;
  struct Ws {
    float *X, *O, *Y1, *Y2, *pooled, *E1, *scratch;
    size_t scratch_floats, floats;
    int bc;  // utterances per forward chunk, by the widest operand (the 4d-wide tensor of level 1)
  };

  void build_params() override;
  Pw fold_pw(const std::string& wname, const std::string& bn, int N, int cin, int taps);
  ConvW fold_gemm(const std::string& wname, const std::string& bn, int N, int cin);
  void finalize() override;
  void check_forward(int B, int T) const override;
  Ws ws_layout(int B, int T, float* base) const;
  size_t ws_floats(int B, int T) const override { return ws_layout(B, T, nullptr).floats; }
  void forward(const float* feats, int B, int T, float* embed, float* ws, hipStream_t s) override;
};
}  // namespace

Model::Impl* make_gemini(const std::string& arch, int feat_dim, int embed_dim, bool emb_bn, bool two_emb) {
  struct Arch {  // gemini_dfresnet.py:145-178
    const char* name;
    int depths[4];
  };
  static const Arch kArchs[] = {{"Gemini_DF_ResNet60", {3, 3, 9, 3}},
                                {"Gemini_DF_ResNet114", {3, 3, 27, 3}},
                                {"Gemini_DF_ResNet183", {3, 8, 45, 3}},
                                {"Gemini_DF_ResNet237", {3, 8, 63, 3}}};
  const Arch* a = std::find_if(std::begin(kArchs), std::end(kArchs), [&](const Arch& k) { return arch == k.name; });
  if (a == std::end(kArchs)) return nullptr;
  WSP_CHECK(!emb_bn, "Gemini DF-ResNet has no emb_bn");
  // gemini_dfresnet.py:63 sizes seg_1 for int(feat_dim / 16) frequency rows while level 4 keeps ceil(feat_dim / 16)
  WSP_CHECK(feat_dim >= 16 && feat_dim % 16 == 0, "Gemini DF-ResNet feat_dim must be a positive multiple of 16");
  WSP_CHECK(embed_dim > 0, "embed_dim must be positive");
  Gemini* g = new Gemini(arch, feat_dim, embed_dim, emb_bn, two_emb);
  std::copy(a->depths, a->depths + 4, g->depths);
  g->opt.x3_variant = 7;  // the 1x1 convs (N = 32 .. 1024, K = 32 .. 1024): 1.74 ms against 1.95 (5) and 1.90 (3)
  return g;
}

// state_dict order: 356 / 680 / 1094 / 1418 entries for 60 / 114 / 183 / 237 (+ 5 with two_emb_layer)
void Gemini::build_params() {
  add("downsample_layers.0.0.weight", {kDims[0], 1, 3, 3});
  add_bn("downsample_layers.0.1", kDims[0]);
  for (int i = 1; i <= 4; ++i) {
    const std::string p = "downsample_layers." + std::to_string(i);
    add(p + ".0.weight", {kDims[i], kDims[i - 1], 3, 3});
    add_bn(p + ".1", kDims[i]);
  }
  for (int li = 0; li < 4; ++li)
    for (int bi = 0; bi < depths[li]; ++bi) {
      Block b;
      b.name = "stages." + std::to_string(li) + "." + std::to_string(bi);
      b.d = kDims[li + 1];
      const int d = b.d;
      add(b.name + ".conv1.weight", {4 * d, d, 1, 1});
      add_bn(b.name + ".bn1", 4 * d);
      add(b.name + ".conv2.weight", {4 * d, 1, 3, 3});
      add_bn(b.name + ".bn2", 4 * d);
      add(b.name + ".conv3.weight", {d, 4 * d, 1, 1});
      add_bn(b.name + ".bn3", d);
      blocks.push_back(b);
    }
  const int stats_dim = (feat_dim / 16) * kDims[4];
  add("seg_1.weight", {embed_dim, stats_dim * 2});
  add("seg_1.bias", {embed_dim});
  if (two_emb) {  // gemini_dfresnet.py:98-100: BatchNorm1d(affine=False) + seg_2
    add("seg_bn_1.running_mean", {embed_dim});
    add("seg_bn_1.running_var", {embed_dim});
    add("seg_bn_1.num_batches_tracked", {});
    add("seg_2.weight", {embed_dim, embed_dim});
    add("seg_2.bias", {embed_dim});
  }
}

// conv [N][cin][taps] -> BN folded, k = tap * cin + c, as 16x16x32 A fragments
Gemini::Pw Gemini::fold_pw(const std::string& wname, const std::string& bn, int N, int cin, int taps) {
  const Folded f = fold_bn(wname, bn);
  Pw pw;
  pw.N = N;
  pw.K = cin * taps;
  const std::vector<float> wk = pack::conv_kmajor(f.w, N, cin, taps, pw.K);
  pw.w = dev.upload_u16(pack::frag16(wk.data(), N, pw.K, pw.K));
  pw.b = dev.upload(f.b);
  return pw;
}

// 1x1 conv [N][cin] -> BN folded, for the shared implicit GEMM
ConvW Gemini::fold_gemm(const std::string& wname, const std::string& bn, int N, int cin) {
  const Folded f = fold_bn(wname, bn);
  return pack_conv(f.w, N, cin, 1, f.b.data(), "");
}

void Gemini::finalize() {
  const Folded stem = fold_bn("downsample_layers.0.0.weight", "downsample_layers.0.1");  // as the ResNets'
  stem_w = dev.upload(stem.w);
  stem_b = dev.upload(stem.b);
  for (int i = 1; i <= 4; ++i) {
    const std::string p = "downsample_layers." + std::to_string(i);
    WSP_CHECK(gemini_down_supported(kDims[i - 1], kDims[i]), "Gemini DF-ResNet: no downsample kernel");
    down[i - 1] = fold_pw(p + ".0.weight", p + ".1", kDims[i], kDims[i - 1], 9);
  }
  for (Block& b : blocks) {
    const int d = b.d, C = 4 * d;
    WSP_CHECK(gemini_dw_supported(C) && gemini_tail_supported(d), "Gemini DF-ResNet: no kernel for width " + std::to_string(d));
    b.c1 = fold_gemm(b.name + ".conv1.weight", b.name + ".bn1", C, d);
    const Folded f2 = fold_bn(b.name + ".conv2.weight", b.name + ".bn2");  // [C][9] -> tap-major [9][C]
    std::vector<float> w2((size_t)9 * C);
    for (int c = 0; c < C; ++c)
      for (int tap = 0; tap < 9; ++tap) w2[(size_t)tap * C + c] = f2.w[(size_t)c * 9 + tap];
    b.w2 = dev.upload(w2);
    b.b2 = dev.upload(f2.b);
    b.c3g = fold_gemm(b.name + ".conv3.weight", b.name + ".bn3", d, C);
    b.c3 = fold_pw(b.name + ".conv3.weight", b.name + ".bn3", d, C, 1);
  }
  // seg_1 over TSTP stats; reference flatten index s*C*F4 + c*F4 + f, ours f*2C + s*C + c
  const int C4 = kDims[4], F4 = feat_dim / 16;
  const auto& W = P("seg_1.weight");
  const int K = 2 * C4 * F4;
  std::vector<float> wp((size_t)embed_dim * K);
  for (int n = 0; n < embed_dim; ++n)
    for (int f = 0; f < F4; ++f)
      for (int sidx = 0; sidx < 2; ++sidx)
        for (int ch = 0; ch < C4; ++ch)
          wp[(size_t)n * K + f * 2 * C4 + sidx * C4 + ch] = W[(size_t)n * K + sidx * C4 * F4 + ch * F4 + f];
  seg1 = pack_lin(wp.data(), embed_dim, K, K, P("seg_1.bias").data());
  if (two_emb) {
    // seg_2(BN(relu(embed_a))), BN without affine: (W2 diag(s)) r + (b2 - W2 (rm s))
    const auto& rm = P("seg_bn_1.running_mean");
    const auto& rv = P("seg_bn_1.running_var");
    const auto& W2 = P("seg_2.weight");
    const auto& b2 = P("seg_2.bias");
    const int D = embed_dim;
    std::vector<float> w2((size_t)D * D), bb(D);
    for (int n = 0; n < D; ++n) {
      double acc = b2[n];
      for (int k = 0; k < D; ++k) {
        const double sk = 1.0 / std::sqrt((double)rv[k] + kBnEps);
        w2[(size_t)n * D + k] = (float)(W2[(size_t)n * D + k] * sk);
        acc -= (double)W2[(size_t)n * D + k] * rm[k] * sk;
      }
      bb[n] = (float)acc;
    }
    seg2 = pack_lin(w2.data(), D, D, D, bb.data());
  }
}

void Gemini::check_forward(int, int T) const {
  // as every family off the f32 GEMM path: the message names the first of them
  WSP_CHECK(opt.precision == 1, "ResNet runs on the bf16x3 kernels only (precision=1)");
  // T' = (T - 1) / 2 + 1 frames reach the pooling, whose unbiased variance needs two
  WSP_CHECK(T >= 3, "Gemini DF-ResNet needs >= 3 frames (2 after the time-stride-2 level)");
}

Gemini::Ws Gemini::ws_layout(int B, int T, float* base) const {
  // floats per utterance: the d-wide ping-pong pair holds the stem's output and every level's,
  // the 4d-wide buffer(s) a block's expanded tensor
  size_t narrow = (size_t)feat_dim * T * kDims[0], wide = 0;
  int Fi = feat_dim, Ti = T;
  for (int li = 0; li < 4; ++li) {
    Fi = (Fi - 1) / 2 + 1;
    Ti = (Ti - 1) / kStrideT[li] + 1;
    const size_t pos = (size_t)Fi * Ti;
    narrow = std::max(narrow, pos * kDims[li + 1]);
    wide = std::max(wide, pos * 4 * kDims[li + 1]);
  }
  const size_t K = (size_t)Fi * 2 * kDims[4];
  WsCursor c{base};
  Ws w;
  w.bc = chunk_for(B, std::max(wide, narrow) * sizeof(float));
  const size_t bc = w.bc;
  w.X = c.take(bc * narrow);
  w.O = c.take(bc * narrow);
  w.Y1 = c.take(bc * wide);
  w.Y2 = opt.ib_fused ? nullptr : c.take(bc * wide);  // the depthwise conv's output, unfused route only
  w.pooled = c.take(bc * K);
  w.E1 = c.take(bc * embed_dim);
  w.scratch_floats = small_linear_scratch_floats((int)bc, embed_dim, (int)K);
  w.scratch = c.take(w.scratch_floats);
  w.floats = c.off;
  return w;
}

void Gemini::forward(const float* feats, int B, int T, float* embed, float* ws, hipStream_t s) {
  const Ws W = ws_layout(B, T, ws);
  const int bc = W.bc;
  const bool fused = opt.ib_fused != 0;
  for (int b0 = 0; b0 < B; b0 += bc) {
    const int nb = std::min(bc, B - b0);
    int Fi = feat_dim, Ti = T;
    run("stem", 0, s,
        [&] { launch_resnet_stem(feats + (size_t)b0 * T * feat_dim, nb, T, feat_dim, kDims[0], stem_w, stem_b, W.X, s); });
    float* x = W.X;
    float* o = W.O;
    size_t ib = 0;
    for (int li = 0; li < 4; ++li) {
      const int d = kDims[li + 1], C = 4 * d;
      const GeminiDownArgs g{x, kDims[li], nb, Fi, Ti, kDims[li], 2, kStrideT[li], down[li].w, down[li].b, d, o, d};
      Fi = (Fi - 1) / 2 + 1;
      Ti = (Ti - 1) / kStrideT[li] + 1;
      const double pos = (double)nb * Fi * Ti;
      run("gem_down", 2.0 * pos * d * down[li].K, s, [&] { launch_gemini_down(g, s); });
      std::swap(x, o);
      for (int bi = 0; bi < depths[li]; ++bi, ++ib) {
        const Block& b = blocks[ib];
        const int M = nb * Fi * Ti;
        gemm("gem_pw1", b.c1, x, d, W.Y1, C, M, M, 1, 0, kActRelu, s, nullptr, 0);
        if (fused) {
          const GeminiTailArgs t{W.Y1, C, nb, Fi, Ti, d, b.w2, b.b2, b.c3.w, b.c3.b, x, d, o, d};
          run("gem_tail", 2.0 * pos * C * (d + 9.0), s, [&] { launch_gemini_tail(t, s); });
        } else {
          const GeminiDwArgs dw{W.Y1, C, nb, Fi, Ti, C, b.w2, b.b2, W.Y2, C};
          run("gem_dw", 2.0 * pos * C * 9.0, s, [&] { launch_gemini_dw(dw, s); });
          ConvGemmArgs g3{};
          one_operand(g3, W.Y2, C, C);
          fill(g3, b.c3g, M, M, 1, 0, o, d, kActRelu, nullptr, true, nullptr, 0);
          g3.res = x;
          g3.ldres = d;
          g3.role = 2;  // the residual loaded ahead of the last k-tiles, as the ResNet's conv3
          run("gem_pw2", 2.0 * pos * C * d, s, [&] { launch(g3, b.c3g, s); });
        }
        std::swap(x, o);
      }
    }
    // TSTP over frames of the last level for every (utterance, freq) row block, then seg_1 (+ seg_2)
    const int Ci = kDims[4];
    run("tstp_head", 0, s, [&] {
      launch_frame_stats(x, Ci, nb * Fi, Ti, Ci, W.pooled, 2 * Ci, 1, Ci, s);
      float* e_out = embed + (size_t)b0 * embed_dim;
      launch_small_linear({W.pooled, Fi * 2 * Ci, seg1.wt, seg1.bias, two_emb ? W.E1 : e_out, embed_dim, nb,
                           Fi * 2 * Ci, embed_dim, two_emb ? 1 : 0, W.scratch_floats ? W.scratch : nullptr,
                           W.scratch_floats},
                          s);
      if (two_emb)
        launch_small_linear({W.E1, embed_dim, seg2.wt, seg2.bias, e_out, embed_dim, nb, embed_dim, embed_dim, 0}, s);
    });
  }
}

}  // namespace wsp
