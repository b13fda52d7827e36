// ResNet (resnet.py:110-260) and SimAM-ResNet (samresnet.py:20-166): parameter tables, BatchNorm
// folding / packing, workspace and the two forward schedules.  The two share the stem, the block
// table (RBlock), the chunk rule, the 2-D implicit GEMM and the 3x3 dispatch; NHWC activations
// [B][F][T][C].
#include "conv3x3_img.h"
#include "model_impl.h"

namespace wsp {

namespace {
// ResNet (resnet.py:110-260), NHWC activations [B][F][T][C]; `simam`: SimAM-ResNet
// (samresnet.py:20-166): basic blocks whose bn2 output passes SimAM before the shortcut add, ASP
// pooling, `bottleneck` Linear.  The stem width is option "in_planes".
struct ResNet final : Model::Impl {
  using Impl::Impl;
  bool simam = false;
  bool bottleneck = true;
  int nblocks[4] = {0, 0, 0, 0};
  float *stem_w = nullptr, *stem_b = nullptr;  // <pre>conv1 + bn1
  bool img_ok(const ConvW& cw, int C) const { return cw.frag && opt.conv3x3_img && (C <= 64 || opt.conv3x3_img >= 2); }
  struct RBlock {
    ConvW c1, c2, c3, sc;
    // conv3 (bn3 folded) and the projection shortcut (its bn folded) as ONE 1x1 GEMM over
    // [y2 | strided x] (K = planes + in_planes, bias b3 + b_sc): the shortcut's output never goes
    // through HBM (option "sc_fuse"; bottleneck blocks off the fused-tail path, N % 256 == 0)
    ConvW c3sc;
    void* w3acc = nullptr;  // conv3 (bn3 folded) as pack_frag_acc B fragments for bottleneck_tail
    // [conv3 | shortcut] (both BN-folded) for the in-tail shortcut (BottleneckTailArgs::xsc) and its
    // summed bias: a stride-1 first block with in_planes == planes == 32
    void* w3scx = nullptr;
    float* b3scx = nullptr;
    void* w1frag = nullptr;  // conv1 (bn1 folded) as pack_frag B fragments: run inside the previous block's tail
    bool has_sc = false;
    int stride = 1, in_planes = 0, planes = 0, out_planes = 0;
    std::string name;    // state_dict prefix, "[front.]layer<li + 1>.<bi>"
    int li = 0, bi = 0;  // stage, block within the stage
  };
  std::vector<RBlock> rblocks;
  LinW seg1, seg2;  // seg2: two_emb_layer's seg_2 with the affine-free seg_bn_1 folded in
  ConvW asp1, asp2;  // SimAM-ResNet: ASP attention, `bottleneck`
  LinW simam_head;
  // one chunk's regions; y1_floats / y2_floats: the (padded) sizes of Y1 / Y2, which the heads reuse
  // as split-K scratch.  From `part` on: SimAM-ResNet only.
  struct Ws {
    float *X, *O, *Y1, *Y2, *SC, *pooled;
    double* part = nullptr;  // f64 moment partials
    float *coef = nullptr, *Xt = nullptr, *att = nullptr, *logit = nullptr;
    size_t y1_floats, y2_floats, floats;
    int bc;  // utterances per forward chunk, by the widest activation operand of any block
  };

  void build_blocks(const std::string& pre, const char* sc_conv, const char* sc_bn);
  void build_params() override;
  bool owns_option(const std::string& key) const override { return simam && key == "in_planes"; }
  ConvW pack_conv_bn(const std::string& wname, const std::string& bn, int N, int cin, int taps,
                     void** acc_frag = nullptr, void** b_frag = nullptr);
  void finalize_blocks(const std::string& pre, const char* sc_conv, const char* sc_bn);
  void finalize() override;
  void finalize_simam();
  void check_forward(int B, int T) const override;
  Ws ws_layout(int B, int T, float* base) const;
  size_t ws_floats(int B, int T) const override { return ws_layout(B, T, nullptr).floats; }
  void gemm2d(const char* tag, const ConvW& cw, const float* a0, int lda, float* out, int ldo, int B, int Fi, int Ti,
              int kw, int stride, int pad, int act, const float* res, int ldres, hipStream_t s);
  void gemm1x1(const char* tag, const ConvW& cw, const float* a0, float* out, int M, int act, const float* res,
               hipStream_t s);
  void gemm_c3sc(const char* tag, const RBlock& rb, const float* y2, const float* x, int Ci, float* out, int B, int Fi,
                 int Ti, int Fo, int To, hipStream_t s);
  void conv3x3(const char* tag, const ConvW& cw, const float* in, int ldin, float* out, int B, int Fi, int Ti,
               int stride, bool relu, const float* res, hipStream_t s);
  void forward(const float* feats, int B, int T, float* embed, float* ws, hipStream_t s) override;
  void forward_simam(const float* feats, int B, int T, float* embed, float* ws, hipStream_t s);
};
}  // namespace

Model::Impl* make_resnet(const std::string& arch, int feat_dim, int embed_dim, bool emb_bn, bool two_emb) {
  // bottleneck?, blocks per stage; SimAM (samresnet.py:124-166): basic SimAM blocks
  struct Arch {
    const char* name;
    bool simam, bottleneck;
    int nblocks[4];
  };
  static const Arch kArchs[] = {
      {"ResNet18", false, false, {2, 2, 2, 2}},           {"ResNet34", false, false, {3, 4, 6, 3}},
      {"ResNet50", false, true, {3, 4, 6, 3}},            {"ResNet101", false, true, {3, 4, 23, 3}},
      {"ResNet152", false, true, {3, 8, 36, 3}},          {"ResNet221", false, true, {6, 16, 48, 3}},
      {"ResNet293", false, true, {10, 20, 64, 3}},        {"SimAM_ResNet34_ASP", true, false, {3, 4, 6, 3}},
      {"SimAM_ResNet100_ASP", true, false, {6, 16, 24, 3}}};
  const Arch* a = std::find_if(std::begin(kArchs), std::end(kArchs), [&](const Arch& k) { return arch == k.name; });
  if (a == std::end(kArchs)) return nullptr;
  if (a->simam) {
    WSP_CHECK(!two_emb && !emb_bn, "SimAM-ResNet has no emb_bn / two_emb_layer");
    WSP_CHECK(feat_dim >= 8 && feat_dim % 8 == 0, "SimAM-ResNet acoustic_dim must be a multiple of 8");
    WSP_CHECK(embed_dim > 0, "embed_dim must be positive");
  } else {
    // resnet.py:124 sizes the pooling for int(feat_dim / 8) frequency rows while stage 4 keeps
    // ceil(feat_dim / 8): the reference model only runs for multiples of 8
    WSP_CHECK(feat_dim >= 8 && feat_dim % 8 == 0, "ResNet feat_dim must be a positive multiple of 8");
  }
  ResNet* m = new ResNet(arch, feat_dim, embed_dim, emb_bn, two_emb);
  m->simam = a->simam;
  m->bottleneck = a->bottleneck;
  std::copy(a->nblocks, a->nblocks + 4, m->nblocks);
  // SimAM: MFMA-bound 3x3 convs (K = 9C): wide tiles where N % 256 == 0 (+6 % over variant 3).
  // Basic blocks: 256 x 128 swizzled (with the residual prefetch, ROLE 2: +1.3 % C3 over variant 3,
  // r2c); bottleneck ResNets: family 7 wherever it takes the operands (1x1 convs with N % 256 == 0),
  // family 6 elsewhere — ResNet293 C3 +0.2-0.4 % over 4 in three interleaved pairs (r6u)
  m->opt.x3_variant = a->simam ? 5 : a->bottleneck ? 7 : 4;
  m->opt.streams = 2;  // two utterance ranges in flight: ResNet293 C3 +8.6 %, SimAM-ResNet100 +3.8 %
  if (a->simam) m->opt.in_planes = 64;  // samresnet.py:124 (option "in_planes" before the weights)
  return m;
}

// Stem and block table under `pre`; a block's projection shortcut is <block>.<sc_conv> / .<sc_bn>.
// Parameter order is the reference state_dict's.
void ResNet::build_blocks(const std::string& pre, const char* sc_conv, const char* sc_bn) {
  const int exp = bottleneck ? 4 : 1, k1 = bottleneck ? 1 : 3;
  add(pre + "conv1.weight", {opt.in_planes, 1, 3, 3});
  add_bn(pre + "bn1", opt.in_planes);
  int in_planes = opt.in_planes;
  for (int li = 0; li < 4; ++li) {
    const int planes = opt.in_planes << li;
    for (int bi = 0; bi < nblocks[li]; ++bi) {
      RBlock rb;
      rb.name = pre + "layer" + std::to_string(li + 1) + "." + std::to_string(bi);
      rb.li = li;
      rb.bi = bi;
      rb.stride = (li > 0 && bi == 0) ? 2 : 1;
      rb.in_planes = in_planes;
      rb.planes = planes;
      rb.out_planes = planes * exp;
      const std::string& p = rb.name;
      add(p + ".conv1.weight", {planes, in_planes, k1, k1});
      add_bn(p + ".bn1", planes);
      add(p + ".conv2.weight", {planes, planes, 3, 3});
      add_bn(p + ".bn2", planes);
      if (bottleneck) {
        add(p + ".conv3.weight", {planes * 4, planes, 1, 1});
        add_bn(p + ".bn3", planes * 4);
      }
      if (rb.stride != 1 || in_planes != rb.out_planes) {
        rb.has_sc = true;
        add(p + "." + sc_conv + ".weight", {rb.out_planes, in_planes, 1, 1});
        add_bn(p + "." + sc_bn, rb.out_planes);
      }
      rblocks.push_back(rb);
      in_planes = rb.out_planes;
    }
  }
}

// state_dict of SimAM_ResNet{34,100}_ASP (samresnet.py:72-166): front.* backbone,
// pooling.attention.{0,2,3} (ASP, pooling_layers.py:151-173), bottleneck.  Rebuilt when option
// "in_planes" changes the stem width.
void ResNet::build_params() {
  params.clear();
  idx.clear();
  rblocks.clear();
  if (simam) {
    build_blocks("front.", "downsample.0", "downsample.1");
    const int CF = 8 * opt.in_planes * (feat_dim / 8);  // ASP: in_planes * 8 * int(acoustic_dim / 8)
    add("pooling.attention.0.weight", {128, CF, 1});
    add("pooling.attention.0.bias", {128});
    add_bn("pooling.attention.2", 128);
    add("pooling.attention.3.weight", {CF, 128, 1});
    add("pooling.attention.3.bias", {CF});
    add("bottleneck.weight", {embed_dim, 2 * CF});
    add("bottleneck.bias", {embed_dim});
    return;
  }
  build_blocks("", "shortcut.0", "shortcut.1");
  const int stats_dim = (feat_dim / 8) * opt.in_planes * 8 * (bottleneck ? 4 : 1);
  add("seg_1.weight", {embed_dim, stats_dim * 2});
  add("seg_1.bias", {embed_dim});
  if (two_emb) {  // resnet.py:158-161: BatchNorm1d(affine=False) + seg_2
    add("seg_bn_1.running_mean", {embed_dim});
    add("seg_bn_1.running_var", {embed_dim});
    add("seg_bn_1.num_batches_tracked", {});
    add("seg_2.weight", {embed_dim, embed_dim});
    add("seg_2.bias", {embed_dim});
  }
}

// conv -> BN (eval) folded into the weights: W' = W * s[n], bias = shift.
ConvW ResNet::pack_conv_bn(const std::string& wname, const std::string& bn, int N, int cin, int taps,
                            void** acc_frag, void** b_frag) {
  const auto [w, b] = fold_bn(wname, bn);
  ConvW cw = pack_conv(w, N, cin, taps, b.data(), "");
  if (acc_frag) *acc_frag = pack_frag_acc(w, N, cin * taps);
  if (b_frag) *b_frag = pack_frag(w, N, cin * taps);
  // conv3x3_img.hip: fragments in the same k = tap * cin + c order as the implicit GEMM's packed image
  if (taps == 9 && N == cin && conv3x3_img_supported(cin))
    cw.frag = pack_frag(pack::conv_kmajor(w, N, cin, 9, 9 * cin), N, 9 * cin);
  return cw;
}

// The stem and every block's convs with their BatchNorms folded in, for both families.
void ResNet::finalize_blocks(const std::string& pre, const char* sc_conv, const char* sc_bn) {
  const Folded stem = fold_bn(pre + "conv1.weight", pre + "bn1");
  stem_w = dev.upload(stem.w);
  stem_b = dev.upload(stem.b);
  for (RBlock& rb : rblocks) {
    const std::string& p = rb.name;
    if (bottleneck) {
      // a stride-1 block whose input has 4 x its planes (every block after the first of a
      // stage) runs its conv1 inside the previous block's bottleneck_tail
      // ... and a stage's first block whose conv1 is 2C <- 4C of the previous stage's C = 32 / 64
      // planes runs it inside the previous stage's last tail (c1_stage_fuse)
      const bool c1_in_tail = (rb.stride == 1 && rb.in_planes == 4 * rb.planes && rb.bi > 0 &&
                               bottleneck_tail_supported(rb.planes)) ||
                              (rb.bi == 0 && rb.li > 0 && rb.in_planes == 2 * rb.planes && rb.planes <= 128 &&
                               bottleneck_tail_supported(rb.planes / 2));
      rb.c1 = pack_conv_bn(p + ".conv1.weight", p + ".bn1", rb.planes, rb.in_planes, 1, nullptr,
                           c1_in_tail ? &rb.w1frag : nullptr);
      rb.c2 = pack_conv_bn(p + ".conv2.weight", p + ".bn2", rb.planes, rb.planes, 9);
      rb.c3 = pack_conv_bn(p + ".conv3.weight", p + ".bn3", rb.out_planes, rb.planes, 1,
                           rb.stride == 1 && bottleneck_tail_supported(rb.planes) ? &rb.w3acc : nullptr);
    } else {
      rb.c1 = pack_conv_bn(p + ".conv1.weight", p + ".bn1", rb.planes, rb.in_planes, 9);
      rb.c2 = pack_conv_bn(p + ".conv2.weight", p + ".bn2", rb.planes, rb.planes, 9);
    }
    if (!rb.has_sc) continue;
    const std::string scw = p + "." + sc_conv + ".weight", scb = p + "." + sc_bn;
    rb.sc = pack_conv_bn(scw, scb, rb.out_planes, rb.in_planes, 1);
    // [conv3 | shortcut], both BN-folded, over K = planes + in_planes with the summed bias: as one
    // GEMM (c3sc) and / or as the fused tail's conv3 (w3scx)
    const bool as_gemm = bottleneck && rb.out_planes % 256 == 0 && rb.planes % 32 == 0 && rb.in_planes % 32 == 0;
    const bool in_tail = bottleneck && rb.stride == 1 && rb.in_planes == rb.planes && rb.planes == 32 && rb.w3acc;
    if (!as_gemm && !in_tail) continue;
    std::vector<double> s3, h3, ss, hs;
    bn_affine(p + ".bn3", s3, h3);
    bn_affine(scb, ss, hs);
    const std::vector<float>& w3 = P(p + ".conv3.weight");
    const std::vector<float>& wsc = P(scw);
    const int K = rb.planes + rb.in_planes, N = rb.out_planes;
    std::vector<float> wf((size_t)N * K), bf(N);
    for (int n = 0; n < N; ++n) {
      for (int k = 0; k < rb.planes; ++k) wf[(size_t)n * K + k] = (float)(w3[(size_t)n * rb.planes + k] * s3[n]);
      for (int k = 0; k < rb.in_planes; ++k)
        wf[(size_t)n * K + rb.planes + k] = (float)(wsc[(size_t)n * rb.in_planes + k] * ss[n]);
      bf[n] = (float)h3[n] + (float)hs[n];
    }
    if (as_gemm) rb.c3sc = pack_conv(wf, N, K, 1, bf.data(), "");
    if (in_tail) {
      rb.w3scx = pack_frag_acc(wf, N, K, rb.planes);
      rb.b3scx = dev.upload(bf);
    }
  }
}

void ResNet::finalize() {
  if (simam) return finalize_simam();
  finalize_blocks("", "shortcut.0", "shortcut.1");
  // seg_1 over TSTP stats; reference flatten index s*C*F4 + c*F4 + f, ours f*2C + s*C + c
  const int C4 = rblocks.back().out_planes, F4 = feat_dim / 8;
  const auto& W = P("seg_1.weight");
  const int K = 2 * C4 * F4;
  std::vector<float> wp((size_t)embed_dim * K);
  for (int n = 0; n < embed_dim; ++n)
    for (int f = 0; f < F4; ++f)
      for (int sidx = 0; sidx < 2; ++sidx)
        for (int c = 0; c < C4; ++c)
          wp[(size_t)n * K + f * 2 * C4 + sidx * C4 + c] = W[(size_t)n * K + sidx * C4 * F4 + c * F4 + f];
  seg1 = pack_lin(wp.data(), embed_dim, K, K, P("seg_1.bias").data());
  if (two_emb) {
    // embed_b = seg_2(BN(relu(embed_a))), BN without affine (resnet.py:196-200):
    // W2 ((r - rm) / sqrt(rv + eps)) + b2 = (W2 diag(s)) r + (b2 - W2 (rm s))
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

void ResNet::finalize_simam() {
  finalize_blocks("front.", "downsample.0", "downsample.1");
  // reference channel index c*F4 + f of x.reshape(B, C*F, T); ours f*C4 + c (frame rows [T][F][C])
  const int C4 = rblocks.back().out_planes, F4 = feat_dim / 8, CF = C4 * F4;
  auto ref_ch = [&](int k) { return (k % C4) * F4 + k / C4; };
  {
    const auto& W = P("pooling.attention.0.weight");
    std::vector<float> wp((size_t)128 * CF);
    for (int n = 0; n < 128; ++n)
      for (int k = 0; k < CF; ++k) wp[(size_t)n * CF + k] = W[(size_t)n * CF + ref_ch(k)];
    asp1 = pack_conv(wp, 128, CF, 1, P("pooling.attention.0.bias").data(), "pooling.attention.2");
  }
  {
    const auto& W = P("pooling.attention.3.weight");
    const auto& bb = P("pooling.attention.3.bias");
    std::vector<float> wp((size_t)CF * 128), bp(CF);
    for (int n = 0; n < CF; ++n) {
      for (int k = 0; k < 128; ++k) wp[(size_t)n * 128 + k] = W[(size_t)ref_ch(n) * 128 + k];
      bp[n] = bb[ref_ch(n)];
    }
    asp2 = pack_conv(wp, CF, 128, 1, bp.data(), "");
  }
  {
    const auto& W = P("bottleneck.weight");
    const int K = 2 * CF;
    std::vector<float> wp((size_t)embed_dim * K);
    for (int n = 0; n < embed_dim; ++n)
      for (int sidx = 0; sidx < 2; ++sidx)
        for (int k = 0; k < CF; ++k) wp[(size_t)n * K + sidx * CF + k] = W[(size_t)n * K + sidx * CF + ref_ch(k)];
    simam_head = pack_lin(wp.data(), embed_dim, K, K, P("bottleneck.bias").data());
  }
}

void ResNet::check_forward(int, int T) const {
  WSP_CHECK(opt.precision == 1, "ResNet runs on the bf16x3 kernels only (precision=1)");
  WSP_CHECK(!simam || (T + 7) / 8 >= 2, "SimAM-ResNet needs >= 2 frames after the three stride-2 stages");
}

ResNet::Ws ResNet::ws_layout(int B, int T, float* base) const {
  struct {
    size_t big = 0, y1 = 0, y2 = 0, sc = 0;  // floats per utterance
    int F4 = 0, T4 = 0, C4 = 0;
  } r;
  int Fi = feat_dim, Ti = T;
  r.big = (size_t)Fi * Ti * opt.in_planes;
  for (const RBlock& rb : rblocks) {
    const int Fo = (Fi - 1) / rb.stride + 1, To = (Ti - 1) / rb.stride + 1;
    r.big = std::max(r.big, (size_t)Fo * To * rb.out_planes);
    r.y1 = std::max(r.y1, (size_t)(bottleneck ? Fi * Ti : Fo * To) * rb.planes);
    r.y2 = std::max(r.y2, (size_t)Fo * To * rb.planes);
    // the buffers Y1 / Y2 alternate as a fused tail's input and its next-conv1 output, which at a
    // stage transition is the next stage's conv1 at this resolution
    if (bottleneck) r.y2 = std::max(r.y2, (size_t)Fi * Ti * rb.planes);
    if (rb.has_sc) r.sc = std::max(r.sc, (size_t)Fo * To * rb.out_planes);
    Fi = Fo;
    Ti = To;
  }
  r.F4 = Fi;
  r.T4 = Ti;
  r.C4 = rblocks.back().out_planes;
  WsCursor c{base};
  Ws w;
  w.bc = chunk_for(B, std::max(r.big, std::max(r.y1, std::max(r.y2, r.sc))) * sizeof(float));
  const size_t bc = w.bc;
  w.X = c.take(bc * r.big);
  w.O = c.take(bc * r.big);
  w.Y1 = c.take(bc * r.y1);
  w.Y2 = c.take(bc * r.y2);
  w.SC = c.take(bc * std::max<size_t>(r.sc, 1));
  w.pooled = c.take(bc * r.F4 * 2 * r.C4);
  w.y1_floats = WsCursor::padded(bc * r.y1);
  w.y2_floats = WsCursor::padded(bc * r.y2);
  if (simam) {
    const size_t CF = (size_t)r.C4 * r.F4, cmax = (size_t)rblocks.back().out_planes;
    const size_t nchunk = (size_t)std::max(1, ceil_div(2048, (int)bc));
    w.part = reinterpret_cast<double*>(c.take(bc * nchunk * 2 * cmax * 2));
    w.coef = c.take(bc * 2 * cmax);    // mean / 1/(4(v+l))
    w.Xt = c.take(bc * r.T4 * CF);     // frame rows [T][F*C]
    w.att = c.take(bc * r.T4 * 128);   // attention hidden
    w.logit = c.take(bc * r.T4 * CF);  // attention logits
  }
  w.floats = c.off;
  return w;
}

void ResNet::gemm2d(const char* tag, const ConvW& cw, const float* a0, int lda, float* out, int ldo, int B, int Fi,
                         int Ti, int kw, int stride, int pad, int act, const float* res, int ldres, hipStream_t s) {
  ConvGemmArgs g{};
  one_operand(g, a0, lda, cw.cin);
  const int Fo = (Fi + 2 * pad - kw) / stride + 1, To = (Ti + 2 * pad - kw) / stride + 1;
  const int M = B * Fo * To;
  fill(g, cw, M, M, 1, pad, out, ldo, act, nullptr, true, nullptr, 0);
  g.conv2d = 1;
  g.Fi = Fi;
  g.Ti = Ti;
  g.Fo = Fo;
  g.To = To;
  g.stride = stride;
  g.kw = kw;
  g.res = res;
  g.ldres = ldres;
  run(tag, 2.0 * M * cw.N * cw.K, s, [&] { launch_conv_gemm_x3(g, cw.whi, cw.wlo, opt.x3_variant, s); });
}

void ResNet::gemm1x1(const char* tag, const ConvW& cw, const float* a0, float* out, int M, int act,
                          const float* res, hipStream_t s) {
  ConvGemmArgs g{};
  one_operand(g, a0, cw.cin, cw.cin);
  fill(g, cw, M, M, 1, 0, out, cw.N, act, nullptr, true, nullptr, 0);
  g.res = res;
  g.ldres = cw.N;
  g.role = res && opt.res_prefetch ? 2 : 0;
  run(tag, 2.0 * M * cw.N * cw.K, s, [&] { launch_conv_gemm_x3(g, cw.whi, cw.wlo, opt.x3_variant, s); });
}

// bottleneck conv3 + projection shortcut as one GEMM (RBlock::c3sc, ConvGemmArgs::sc2d): A segment 0
// = y2 [M][planes] (row m), segment 1 = the block input x [B][Fi][Ti][Ci] at the shortcut's
// strided position of output row m
void ResNet::gemm_c3sc(const char* tag, const RBlock& rb, const float* y2, const float* x, int Ci, float* out,
                            int B, int Fi, int Ti, int Fo, int To, hipStream_t s) {
  const ConvW& cw = rb.c3sc;
  ConvGemmArgs g{};
  g.a[0] = y2;
  g.a[1] = g.a[2] = x;
  g.lda[0] = rb.planes;
  g.lda[1] = g.lda[2] = Ci;
  g.cseg[0] = 0;
  g.cseg[1] = rb.planes;
  g.cseg[2] = g.cseg[3] = cw.cin;
  const int M = B * Fo * To;
  fill(g, cw, M, M, 1, 0, out, cw.N, kActRelu, nullptr, true, nullptr, 0);
  g.sc2d = 1;
  g.Fi = Fi;
  g.Ti = Ti;
  g.Fo = Fo;
  g.To = To;
  g.stride = rb.stride;
  run(tag, 2.0 * M * cw.N * cw.K, s, [&] { launch_conv_gemm_x3(g, cw.whi, cw.wlo, opt.x3_variant, s); });
}

// BN-folded 3x3 conv, pad 1, N = cw.N output channels (+ res, then ReLU if relu): the image kernel
// (conv3x3_img.hip) for a stride-1 conv it supports (img_ok), else the implicit GEMM
void ResNet::conv3x3(const char* tag, const ConvW& cw, const float* in, int ldin, float* out, int B, int Fi,
                          int Ti, int stride, bool relu, const float* res, hipStream_t s) {
  if (stride == 1 && img_ok(cw, cw.N)) {
    const Conv3x3Args a{in, out, B, Fi, Ti, cw.frag, cw.bias, cw.scale, cw.shift, res, relu, opt.conv3x3_img};
    run(tag, 2.0 * B * Fi * Ti * cw.N * cw.K, s, [&] { launch_conv3x3_img(a, cw.N, s); });
  } else {
    gemm2d(tag, cw, in, ldin, out, cw.N, B, Fi, Ti, 3, stride, 1, relu ? kActRelu : kActNone, res, res ? cw.N : 0, s);
  }
}

void ResNet::forward(const float* feats, int B, int T, float* embed, float* ws, hipStream_t s) {
  if (simam) return forward_simam(feats, B, T, embed, ws, s);
  const Ws W = ws_layout(B, T, ws);
  const int bc = W.bc;
  float *Y1 = W.Y1, *Y2 = W.Y2;
  for (int b0 = 0; b0 < B; b0 += bc) {
    const int nb = std::min(bc, B - b0);
    int Fi = feat_dim, Ti = T, Ci = opt.in_planes;
    run("stem", 0, s, [&] {
      launch_resnet_stem(feats + (size_t)b0 * T * feat_dim, nb, T, feat_dim, opt.in_planes, stem_w, stem_b, W.X, s);
    });
    float* x = W.X;
    float* o = W.O;
    // profiling sub-classes per stage: res_conv1x1.{c1,c3}.L<n>, res_conv3x3.L<n>
    static const char* kC1[4] = {"res_conv1x1.c1.L1", "res_conv1x1.c1.L2", "res_conv1x1.c1.L3",
                                 "res_conv1x1.c1.L4"};
    static const char* kC3[4] = {"res_conv1x1.c3.L1", "res_conv1x1.c3.L2", "res_conv1x1.c3.L3",
                                 "res_conv1x1.c3.L4"};
    static const char* kK3[4] = {"res_conv3x3.L1", "res_conv3x3.L2", "res_conv3x3.L3", "res_conv3x3.L4"};
    static const char* kTl[4] = {"res_tail.L1", "res_tail.L2", "res_tail.L3", "res_tail.L4"};
    bool y1_ready = false;  // this block's conv1 output was written by the previous block's tail
    float* y1_next = nullptr;
    for (size_t ib = 0; ib < rblocks.size(); ++ib) {
      const RBlock& rb = rblocks[ib];
      const int li = rb.li;
      const int Fo = (Fi - 1) / rb.stride + 1, To = (Ti - 1) / rb.stride + 1;
      const float* res = x;
      const bool tail = bottleneck && rb.stride == 1 && opt.res_tail && rb.w3acc && img_ok(rb.c2, rb.planes);
      const RBlock* nx = ib + 1 < rblocks.size() ? &rblocks[ib + 1] : nullptr;
      // the tail also runs the next block's conv1 on this block's output (res_tail 1; the next
      // block's conv2 reads y1 from either buffer); at a stage transition the next (first)
      // block's conv1 is 4C -> 2C at this stage's resolution (option c1_stage_fuse)
      const bool fuse1 =
          tail && opt.res_tail == 1 && nx && nx->w1frag &&
          ((nx->planes == rb.planes && nx->w3acc && nx->stride == 1 && img_ok(nx->c2, nx->planes)) ||
           (opt.c1_stage_fuse && nx->planes == 2 * rb.planes && nx->in_planes == rb.out_planes && rb.planes <= 64));
      // conv3 + shortcut in one GEMM on the non-tail path (sc_fuse): no SC round trip through HBM
      const bool fuse_sc = bottleneck && rb.has_sc && !tail && (opt.sc_fuse & 1) && rb.c3sc.w && opt.x3_variant == 7;
      // ... and inside the tail's conv3 for a stride-1 first block of 32 planes (w3scx)
      const bool tail_sc = fuse1 && (opt.sc_fuse & 2) && rb.w3scx && nx->planes == rb.planes;
      if (rb.has_sc && !fuse_sc && !tail_sc) {
        gemm2d("shortcut", rb.sc, x, Ci, W.SC, rb.out_planes, nb, Fi, Ti, 1, rb.stride, 0, kActNone, nullptr, 0, s);
        res = W.SC;
      }
      if (bottleneck) {
        if (!y1_ready) gemm1x1(kC1[li], rb.c1, x, Y1, nb * Fi * Ti, kActRelu, nullptr, s);
        const float* y1 = y1_ready ? y1_next : Y1;
        y1_ready = false;
        if (tail) {
          // conv2 + conv3 + residual in one launch, y2 in registers (bottleneck_tail); with
          // fuse1 also the next block's conv1 on this block's output (into the buffer the tail
          // does not read)
          BottleneckTailArgs a{y1, res, o, nb, Fi, Ti, rb.c2.frag, rb.c2.bias, rb.w3acc, rb.c3.bias};
          float* y1n = y1 == Y1 ? Y2 : Y1;
          if (fuse1) {
            a.w1n = nx->w1frag;
            a.b1n = nx->c1.bias;
            a.y1n = y1n;
            a.c1n = nx->planes;
          }
          if (tail_sc) {
            a.res = nullptr;
            a.xsc = x;
            a.w3 = rb.w3scx;
            a.b3 = rb.b3scx;
          }
          const double pos = (double)nb * Fi * Ti;
          run(kTl[li],
              2.0 * pos *
                  (rb.c2.N * rb.c2.K + rb.c3.N * rb.c3.K + (fuse1 ? nx->c1.N * nx->c1.K : 0) +
                   (tail_sc ? rb.sc.N * rb.sc.K : 0)),
              s, [&] { launch_bottleneck_tail(a, rb.planes, s); });
          if (fuse1) {
            y1_ready = true;
            y1_next = y1n;
          }
        } else {
          // y1 is in Y1, or in Y2 when the previous block's tail computed this conv1
          float* y2 = y1 == Y2 ? Y1 : Y2;
          conv3x3(kK3[li], rb.c2, y1, rb.planes, y2, nb, Fi, Ti, rb.stride, true, nullptr, s);
          if (fuse_sc)
            gemm_c3sc(kC3[li], rb, y2, x, Ci, o, nb, Fi, Ti, Fo, To, s);
          else
            gemm1x1(kC3[li], rb.c3, y2, o, nb * Fo * To, kActRelu, res, s);
        }
      } else {
        conv3x3(kK3[li], rb.c1, x, Ci, Y1, nb, Fi, Ti, rb.stride, true, nullptr, s);
        conv3x3(kK3[li], rb.c2, Y1, rb.planes, o, nb, Fo, To, 1, true, res, s);
      }
      std::swap(x, o);
      Fi = Fo;
      Ti = To;
      Ci = rb.out_planes;
    }
    // TSTP over frames for every (utterance, freq) row block, then seg_1
    run("tstp_head", 0, s, [&] {
      launch_frame_stats(x, Ci, nb * Fi, Ti, Ci, W.pooled, 2 * Ci, 1, Ci, s);
      float* e_out = embed + (size_t)b0 * embed_dim;
      // split-K partials of seg_1 (K = F/8 x 2 x C) in the free second conv1 buffer; two_emb:
      // relu(seg_1(stats)) into the free conv1 buffer, then the folded seg_bn_1 + seg_2
      launch_small_linear({W.pooled, Fi * 2 * Ci, seg1.wt, seg1.bias, two_emb ? Y1 : e_out, embed_dim, nb, Fi * 2 * Ci,
                           embed_dim, two_emb ? 1 : 0, Y2, W.y2_floats},
                          s);
      if (two_emb)
        launch_small_linear({Y1, embed_dim, seg2.wt, seg2.bias, e_out, embed_dim, nb, embed_dim, embed_dim, 0}, s);
    });
  }
}

void ResNet::forward_simam(const float* feats, int B, int T, float* embed, float* ws, hipStream_t s) {
  const Ws W = ws_layout(B, T, ws);
  const int bc = W.bc;
  float *Y1 = W.Y1, *Z = W.Y2, *Xt = W.Xt;
  for (int b0 = 0; b0 < B; b0 += bc) {
    const int nb = std::min(bc, B - b0);
    int Fi = feat_dim, Ti = T, Ci = opt.in_planes;
    run("stem", 0, s, [&] {
      launch_resnet_stem(feats + (size_t)b0 * T * feat_dim, nb, T, feat_dim, opt.in_planes, stem_w, stem_b, W.X, s);
    });
    float* x = W.X;
    float* o = W.O;
    for (const RBlock& rb : rblocks) {
      const int Fo = (Fi - 1) / rb.stride + 1, To = (Ti - 1) / rb.stride + 1;
      const float* res = x;
      if (rb.has_sc) {
        gemm2d("shortcut", rb.sc, x, Ci, W.SC, rb.planes, nb, Fi, Ti, 1, rb.stride, 0, kActNone, nullptr, 0, s);
        res = W.SC;
      }
      conv3x3("res_conv3x3", rb.c1, x, Ci, Y1, nb, Fi, Ti, rb.stride, true, nullptr, s);
      conv3x3("res_conv3x3", rb.c2, Y1, rb.planes, Z, nb, Fo, To, 1, false, nullptr, s);
      run("simam", 0, s, [&] { launch_simam(Z, res, o, nb, Fo * To, rb.planes, W.part, W.coef, s); });
      std::swap(x, o);
      Fi = Fo;
      Ti = To;
      Ci = rb.planes;
    }
    const int CF = Fi * Ci;
    run("asp_rows", 0, s, [&] { launch_nhwc_to_tfc(x, Xt, nb, Fi, Ti, Ci, s); });
    gemm("asp_linear1", asp1, Xt, CF, W.att, 128, nb * Ti, Ti, 1, 0, kActRelu, s, nullptr, 0);
    gemm("asp_linear2", asp2, W.att, 128, W.logit, CF, nb * Ti, Ti, 1, 0, kActNone, s, nullptr, 0);
    run("asp_pool_head", 0, s, [&] {
      launch_astp_pool(W.logit, Xt, nb, Ti, CF, W.pooled, s, nullptr, 1e-5f);
      // split-K partials in the free conv1 buffer
      launch_small_linear({W.pooled, 2 * CF, simam_head.wt, simam_head.bias, embed + (size_t)b0 * embed_dim, embed_dim,
                           nb, 2 * CF, embed_dim, 0, Y1, W.y1_floats},
                          s);
    });
  }
}

}  // namespace wsp
