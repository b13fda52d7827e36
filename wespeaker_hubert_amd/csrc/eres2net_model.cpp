// ERes2Net (eres2net.py:75-430): parameter table, BatchNorm folds / packing, workspace and the
// forward schedule.  NHWC activations [B][F][T][C].  A block is conv1 (1x1, strided) -> the Res2
// chain over `scale` channel slices `width` wide (stages 1-2: sp + spx[i] inside the 3x3 kernel;
// stages 3-4: the AFF gate in its own launch) -> conv3 (1x1) + shortcut; every activation but the
// stem's ReLU is clamp(., 0, 20).  The 1x1 convs, the 3x3 steps and the AFF run on eres2net.hip
// (the clamp sits in those kernels' epilogues: the conv-GEMM tile families have no such
// activation); the stem, the three bottom-up downsample convs (2-D implicit GEMM) and the TSTP
// head are the ResNet's.  The four hyper-parameters (m_channels, baseWidth, scale, expansion) are
// data: Base, Large and aug share every line below.
#include "eres2net.h"
#include "model_impl.h"
#include "pw_fold.h"

namespace wsp {

namespace {
constexpr int kBlocks[4] = {3, 4, 6, 3};

struct Eres2Net final : Model::Impl {
  using Impl::Impl;
  int m = 32, base_width = 32, scale = 2, expansion = 2;
  float *stem_w = nullptr, *stem_b = nullptr;  // conv1 + bn1
  struct Aff {  // both BatchNorms folded into the convs
    int C = 0;
    void *wa = nullptr, *wb = nullptr;
    float *ba = nullptr, *bb = nullptr;
  };
  struct Block {
    std::string name;
    int li = 0, in_planes = 0, planes = 0, width = 0, stride = 1, out_planes = 0;
    bool aff = false, has_sc = false;
    Pw c1, c3, sc;
    std::vector<Pw> convs;  // the `scale` 3x3 steps (stages 3-4: conv2_1 first)
    std::vector<Aff> affs;  // stages 3-4: in front of steps 1 .. scale - 1
  };
  std::vector<Block> blocks;
  ConvW down[3];  // layerN_downsample: 3x3 stride 2, no bias
  Aff fuse[3];    // fuse_mode12 / 123 / 1234
  LinW seg1, seg2;
  struct Ws {
    float *X, *O, *Y1, *Y2, *Z, *SC, *D, *FU, *pooled, *E1, *scratch;
    size_t scratch_floats, floats;
    int bc;  // utterances per forward chunk, by the widest activation operand (a stage-1 block output)
  };

  void build_params() override;
  void add_aff(const std::string& p, int C);
  Aff fold_aff(const std::string& p, int C);
  void finalize() override;
  void check_forward(int B, int T) const override;
  Ws ws_layout(int B, int T, float* base) const;
  size_t ws_floats(int B, int T) const override { return ws_layout(B, T, nullptr).floats; }
  void forward(const float* feats, int B, int T, float* embed, float* ws, hipStream_t s) override;
};
}  // namespace

Model::Impl* make_eres2net(const std::string& arch, int feat_dim, int embed_dim, bool emb_bn, bool two_emb) {
  // m_channels, baseWidth, scale, expansion (eres2net.py:394-430)
  struct Arch {
    const char* name;
    int m, base_width, scale, expansion;
  };
  static const Arch kArchs[] = {
      {"ERes2Net34_Base", 32, 32, 2, 2}, {"ERes2Net34_Large", 64, 32, 2, 2}, {"ERes2Net34_aug", 64, 24, 3, 4}};
  const Arch* a = std::find_if(std::begin(kArchs), std::end(kArchs), [&](const Arch& k) { return arch == k.name; });
  if (a == std::end(kArchs)) return nullptr;
  WSP_CHECK(!emb_bn, "ERes2Net has no emb_bn");
  // eres2net.py:261 sizes seg_1 for int(feat_dim / 8) frequency rows while stage 4 keeps ceil(feat_dim / 8)
  WSP_CHECK(feat_dim >= 8 && feat_dim % 8 == 0, "ERes2Net feat_dim must be a positive multiple of 8");
  WSP_CHECK(embed_dim > 0, "embed_dim must be positive");
  Eres2Net* e = new Eres2Net(arch, feat_dim, embed_dim, emb_bn, two_emb);
  e->m = a->m;
  e->base_width = a->base_width;
  e->scale = a->scale;
  e->expansion = a->expansion;
  e->opt.x3_variant = 4;  // the downsample convs (N = 128 .. 2048): 256 x 128 tiles, as the basic-block ResNets
  return e;
}

void Eres2Net::add_aff(const std::string& p, int C) {
  add(p + ".local_att.0.weight", {C / 4, 2 * C, 1, 1});
  add(p + ".local_att.0.bias", {C / 4});
  add_bn(p + ".local_att.1", C / 4);
  add(p + ".local_att.3.weight", {C, C / 4, 1, 1});
  add(p + ".local_att.3.bias", {C});
  add_bn(p + ".local_att.4", C);
}

// state_dict order of ERes2Net (587 entries for scale 2, 809 for aug; + 5 with two_emb_layer)
void Eres2Net::build_params() {
  add("conv1.weight", {m, 1, 3, 3});
  add_bn("bn1", m);
  int in_planes = m;
  for (int li = 0; li < 4; ++li) {
    const int planes = m << li;
    for (int bi = 0; bi < kBlocks[li]; ++bi) {
      Block b;
      b.name = "layer" + std::to_string(li + 1) + "." + std::to_string(bi);
      b.li = li;
      b.in_planes = in_planes;
      b.planes = planes;
      b.width = planes * base_width / 64;
      b.stride = (li > 0 && bi == 0) ? 2 : 1;
      b.out_planes = planes * expansion;
      b.aff = li >= 2;
      b.has_sc = b.stride != 1 || in_planes != b.out_planes;
      const std::string& p = b.name;
      const int w = b.width;
      add(p + ".conv1.weight", {w * scale, in_planes, 1, 1});
      add_bn(p + ".bn1", w * scale);
      if (b.aff) {
        add(p + ".conv2_1.weight", {w, w, 3, 3});
        add_bn(p + ".bn2_1", w);
      }
      const int nconv = b.aff ? scale - 1 : scale;
      for (int i = 0; i < nconv; ++i) add(p + ".convs." + std::to_string(i) + ".weight", {w, w, 3, 3});
      for (int i = 0; i < nconv; ++i) add_bn(p + ".bns." + std::to_string(i), w);
      if (b.aff)
        for (int i = 0; i < nconv; ++i) add_aff(p + ".fuse_models." + std::to_string(i), w);
      add(p + ".conv3.weight", {b.out_planes, w * scale, 1, 1});
      add_bn(p + ".bn3", b.out_planes);
      if (b.has_sc) {
        add(p + ".shortcut.0.weight", {b.out_planes, in_planes, 1, 1});
        add_bn(p + ".shortcut.1", b.out_planes);
      }
      blocks.push_back(b);
      in_planes = b.out_planes;
    }
  }
  const int c = m * expansion;
  for (int i = 1; i <= 3; ++i)
    add("layer" + std::to_string(i) + "_downsample.weight", {c << i, c << (i - 1), 3, 3});
  add_aff("fuse_mode12", c * 2);
  add_aff("fuse_mode123", c * 4);
  add_aff("fuse_mode1234", c * 8);
  const int stats_dim = (feat_dim / 8) * m * 8 * expansion;
  add("seg_1.weight", {embed_dim, stats_dim * 2});
  add("seg_1.bias", {embed_dim});
  if (two_emb) {  // eres2net.py:330-332: BatchNorm1d(affine=False) + seg_2
    add("seg_bn_1.running_mean", {embed_dim});
    add("seg_bn_1.running_var", {embed_dim});
    add("seg_bn_1.num_batches_tracked", {});
    add("seg_2.weight", {embed_dim, embed_dim});
    add("seg_2.bias", {embed_dim});
  }
}

// BN(conv(x) + bias) = (W s) x + (bias s + shift), for both convs of local_att
Eres2Net::Aff Eres2Net::fold_aff(const std::string& p, int C) {
  WSP_CHECK(eres_aff_supported(C), "ERes2Net: no AFF kernel for " + std::to_string(C) + " channels");
  const int H = C / 4, Hp = round_up(H, 32);
  std::vector<double> s1, h1, s2, h2;
  bn_affine(p + ".local_att.1", s1, h1);
  bn_affine(p + ".local_att.4", s2, h2);
  const auto& Wa = P(p + ".local_att.0.weight");
  const auto& Ba = P(p + ".local_att.0.bias");
  const auto& Wb = P(p + ".local_att.3.weight");
  const auto& Bb = P(p + ".local_att.3.bias");
  std::vector<float> wa((size_t)Hp * 2 * C, 0.f), ba(Hp, 0.f), wb((size_t)C * Hp, 0.f), bb(C);
  for (int n = 0; n < H; ++n) {
    for (int k = 0; k < 2 * C; ++k) wa[(size_t)n * 2 * C + k] = (float)(Wa[(size_t)n * 2 * C + k] * s1[n]);
    ba[n] = (float)(Ba[n] * s1[n] + h1[n]);
  }
  for (int n = 0; n < C; ++n) {
    for (int k = 0; k < H; ++k) wb[(size_t)n * Hp + k] = (float)(Wb[(size_t)n * H + k] * s2[n]);
    bb[n] = (float)(Bb[n] * s2[n] + h2[n]);
  }
  Aff a;
  a.C = C;
  a.wa = dev.upload_u16(pack::frag16(wa.data(), Hp, 2 * C, 2 * C));
  a.ba = dev.upload(ba);
  a.wb = dev.upload_u16(pack::frag16(wb.data(), C, Hp, Hp, true));
  a.bb = dev.upload(bb);
  return a;
}

void Eres2Net::finalize() {
  const Folded stem = fold_bn("conv1.weight", "bn1");  // as the ResNets'
  stem_w = dev.upload(stem.w);
  stem_b = dev.upload(stem.b);
  for (Block& b : blocks) {
    const std::string& p = b.name;
    const int w = b.width;
    WSP_CHECK(eres_conv3x3_supported(w), "ERes2Net: no 3x3 kernel for width " + std::to_string(w));
    b.c1 = fold_pw(*this, p + ".conv1.weight", p + ".bn1", w * scale, b.in_planes, 1);
    for (int i = 0; i < scale; ++i) {
      if (b.aff && i == 0) {
        b.convs.push_back(fold_pw(*this, p + ".conv2_1.weight", p + ".bn2_1", w, w, 9));
        continue;
      }
      const std::string n = std::to_string(b.aff ? i - 1 : i);
      b.convs.push_back(fold_pw(*this, p + ".convs." + n + ".weight", p + ".bns." + n, w, w, 9));
      if (b.aff) b.affs.push_back(fold_aff(p + ".fuse_models." + n, w));
    }
    b.c3 = fold_pw(*this, p + ".conv3.weight", p + ".bn3", b.out_planes, w * scale, 1);
    if (b.has_sc) b.sc = fold_pw(*this, p + ".shortcut.0.weight", p + ".shortcut.1", b.out_planes, b.in_planes, 1);
  }
  const int c = m * expansion;
  static const char* kFuse[3] = {"fuse_mode12", "fuse_mode123", "fuse_mode1234"};
  for (int i = 0; i < 3; ++i) {
    down[i] = pack_conv(P("layer" + std::to_string(i + 1) + "_downsample.weight"), c << (i + 1), c << i, 9, nullptr, "");
    fuse[i] = fold_aff(kFuse[i], c << (i + 1));
  }
  // seg_1 over TSTP stats; reference flatten index s*C*F4 + c*F4 + f, ours f*2C + s*C + c
  const int C4 = c * 8, F4 = feat_dim / 8;
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

void Eres2Net::check_forward(int, int T) const {
  // as every family off the f32 GEMM path: the message names the first of them
  WSP_CHECK(opt.precision == 1, "ResNet runs on the bf16x3 kernels only (precision=1)");
  WSP_CHECK((T + 7) / 8 >= 2, "ERes2Net needs >= 9 frames (2 after the three stride-2 stages)");
}

Eres2Net::Ws Eres2Net::ws_layout(int B, int T, float* base) const {
  // floats per utterance
  size_t big = 0, y = 0, z = 0, sc = 0, dn = 0;
  int Fi = feat_dim, Ti = T;
  big = (size_t)Fi * Ti * m;
  for (const Block& b : blocks) {
    Fi = (Fi - 1) / b.stride + 1;
    Ti = (Ti - 1) / b.stride + 1;
    const size_t pos = (size_t)Fi * Ti;
    big = std::max(big, pos * b.out_planes);
    y = std::max(y, pos * b.width * scale);
    if (b.aff) z = std::max(z, pos * b.width);
    if (b.has_sc) sc = std::max(sc, pos * b.out_planes);
    if (b.li >= 1) dn = std::max(dn, pos * b.out_planes);  // a downsample / fuse output has its stage's shape
  }
  const size_t C4 = (size_t)m * expansion * 8, K = (size_t)Fi * 2 * C4;
  WsCursor c{base};
  Ws w;
  w.bc = chunk_for(B, std::max(big, std::max(y, sc)) * sizeof(float));
  const size_t bc = w.bc;
  w.X = c.take(bc * big);
  w.O = c.take(bc * big);
  w.Y1 = c.take(bc * y);
  w.Y2 = c.take(bc * y);
  w.Z = c.take(bc * z);
  w.SC = c.take(bc * sc);
  w.D = c.take(bc * dn);
  w.FU = c.take(bc * dn);
  w.pooled = c.take(bc * K);
  w.E1 = c.take(bc * embed_dim);
  w.scratch_floats = small_linear_scratch_floats((int)bc, embed_dim, (int)K);
  w.scratch = c.take(w.scratch_floats);
  w.floats = c.off;
  return w;
}

void Eres2Net::forward(const float* feats, int B, int T, float* embed, float* ws, hipStream_t s) {
  const Ws W = ws_layout(B, T, ws);
  const int bc = W.bc;
  float *Y1 = W.Y1, *Y2 = W.Y2;
  auto pw = [&](const char* tag, const Pw& w, const float* in, int Ci, int nb, int Fi, int Ti, int stride, float* out,
                const float* res, int act) {
    const EresConvArgs a{in, Ci, nullptr, 0, nb, Fi, Ti, Ci, stride, w.w, w.b, w.N, res, res ? w.N : 0, out, w.N, act};
    const double pos = (double)nb * ((Fi - 1) / stride + 1) * ((Ti - 1) / stride + 1);
    run(tag, 2.0 * pos * w.N * w.K, s, [&] { launch_eres_pw(a, s); });
  };
  auto aff = [&](const Aff& f, const float* x, int ldx, const float* y, int ldy, int M, float* out, int ldo) {
    const EresAffArgs a{x, ldx, y, ldy, M, f.C, f.wa, f.ba, f.wb, f.bb, out, ldo};
    run("eres_aff", 2.0 * M * (2.0 * f.C * (f.C / 4) + (double)(f.C / 4) * f.C), s, [&] { launch_eres_aff(a, s); });
  };
  for (int b0 = 0; b0 < B; b0 += bc) {
    const int nb = std::min(bc, B - b0);
    int Fi = feat_dim, Ti = T, Ci = m;
    run("stem", 0, s,
        [&] { launch_resnet_stem(feats + (size_t)b0 * T * feat_dim, nb, T, feat_dim, m, stem_w, stem_b, W.X, s); });
    float* x = W.X;
    float* o = W.O;
    for (size_t ib = 0; ib < blocks.size(); ++ib) {
      const Block& b = blocks[ib];
      const int Fo = (Fi - 1) / b.stride + 1, To = (Ti - 1) / b.stride + 1;
      const int M = nb * Fo * To, w = b.width, wcat = w * scale;
      const float* res = x;
      if (b.has_sc) {
        pw("eres_pw.sc", b.sc, x, Ci, nb, Fi, Ti, b.stride, W.SC, nullptr, kEresNone);
        res = W.SC;
      }
      pw("eres_pw.c1", b.c1, x, Ci, nb, Fi, Ti, b.stride, Y1, nullptr, kEresClamp);
      // the Res2 chain: step i reads slice i of Y1 (with the previous step's output, slice i - 1
      // of Y2) and writes slice i of Y2, the block's concatenation
      for (int i = 0; i < scale; ++i) {
        EresConvArgs a{Y1, wcat, nullptr, 0, nb, Fo, To, w, 1, b.convs[i].w, b.convs[i].b, w, nullptr, 0,
                       Y2 + i * w, wcat, kEresClamp};
        if (i > 0 && b.aff) {
          aff(b.affs[i - 1], Y2 + (i - 1) * w, wcat, Y1 + i * w, wcat, M, W.Z, w);
          a.a = W.Z;
          a.lda = w;
        } else if (i > 0) {
          a.a = Y2 + (i - 1) * w;
          a.a2 = Y1 + i * w;
          a.lda2 = wcat;
        }
        run("eres_conv3x3", 2.0 * M * w * 9.0 * w, s, [&] { launch_eres_conv3x3(a, s); });
      }
      pw("eres_pw.c3", b.c3, Y2, wcat, nb, Fo, To, 1, o, res, kEresClamp);
      std::swap(x, o);
      Fi = Fo;
      Ti = To;
      Ci = b.out_planes;
      if (ib + 1 < blocks.size() && blocks[ib + 1].li == b.li) continue;
      // ---- end of a stage: the bottom-up path.  fuse = AFF(this stage's output, downsample of
      // the previous fuse); the next downsample (stage 1: of the stage's own output) runs at once.
      // D and FU are this path's own buffers, so the next stage's blocks leave them alone
      if (b.li >= 1) aff(fuse[b.li - 1], x, Ci, W.D, Ci, M, W.FU, Ci);
      if (b.li <= 2) {
        const ConvW& cw = down[b.li];
        const float* src = b.li == 0 ? x : W.FU;
        ConvGemmArgs g{};
        one_operand(g, src, Ci, cw.cin);
        const int Fd = (Fi - 1) / 2 + 1, Td = (Ti - 1) / 2 + 1, Md = nb * Fd * Td;
        fill(g, cw, Md, Md, 1, 1, W.D, cw.N, kActNone, nullptr, false, nullptr, 0);
        g.conv2d = 1;
        g.Fi = Fi;
        g.Ti = Ti;
        g.Fo = Fd;
        g.To = Td;
        g.stride = 2;
        g.kw = 3;
        run("eres_down", 2.0 * Md * cw.N * cw.K, s, [&] { launch_conv_gemm_x3(g, cw.whi, cw.wlo, opt.x3_variant, s); });
      }
    }
    // TSTP over frames of fuse1234 for every (utterance, freq) row block, then seg_1 (+ seg_2)
    run("tstp_head", 0, s, [&] {
      launch_frame_stats(W.FU, Ci, nb * Fi, Ti, Ci, W.pooled, 2 * Ci, 1, Ci, s);
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
