// Res2Net (res2net.py:34-211): parameter table, BatchNorm folds / packing, workspace and the forward
// schedule.  NHWC activations [B][F][T][C].  A block (expansion 2, baseWidth 32, scale 2: width =
// planes / 2) is conv1 (1x1, strided) -> y [M][2w]; s = the 3x3 conv of y[:, :w]; conv3 (1x1) over
// [s | y[:, w:]] + shortcut; every activation but the stem's ReLU is clamp(., 0, 20).  The second
// slice bypasses the 3x3 conv, so the block is not a case of ERes2Net's chain.  Two schedules of the
// tail behind conv1 (option res2_tail):
//   unfused  launch_eres_conv3x3 on y[:, :w] -> S [M][w], then launch_eres_pw with ksplit = w over
//            the concatenated operand [S | Y1[:, w:]]
//   fused    launch_res2_tail (res2net.hip): both products in one launch, s kept in registers
// res2_tail = 0: unfused everywhere; 1 (default): fused in the stages where it measured faster
// (kArchs below, DESIGN.md has the table); 2: fused everywhere (the A/B runs and the tests).
// The stem, the TSTP head and seg_1 / seg_2 are the ResNet's, as in ERes2Net.
#include "eres2net.h"
#include "model_impl.h"
#include "pw_fold.h"
#include "res2net.h"

namespace wsp {

namespace {
constexpr int kBlocks[4] = {3, 4, 6, 3};
constexpr int kExpansion = 2;

struct Arch {
  const char* name;
  int m;
  bool tail[4];  // the stages whose tail ships fused (scripts/res2net_timing.py)
};
// fused where its summed tail time was lower in all three interleaved pairs at T = 200 and at T = 500
// (B = 64): Base stage 4 and Large stages 3 - 4 lose at T = 200 (a grid of one 16-position wave per
// SIMD on w = 128 / 256 streams the 3x3 weights from L2 once per 16 positions)
const Arch kArchs[] = {{"Res2Net34_Base", 32, {true, true, true, false}},
                       {"Res2Net34_Large", 64, {true, true, false, false}}};

struct Res2Net final : Model::Impl {
  using Impl::Impl;
  int m = 32;
  bool tail_stage[4] = {false, false, false, false};
  float *stem_w = nullptr, *stem_b = nullptr;  // conv1 + bn1
  struct Block {
    std::string name;
    int li = 0, in_planes = 0, width = 0, stride = 1, out_planes = 0;
    bool has_sc = false;
    Pw c1, c2, c3, c3t, sc;  // c3t: conv3 in acc order, for the fused tail
  };
  std::vector<Block> blocks;
  LinW seg1, seg2;
  struct Ws {
    float *X, *O, *Y1, *S, *SC, *pooled, *E1, *scratch;
    size_t scratch_floats, floats;
    int bc;  // utterances per forward chunk, by the widest activation operand (a stage-1 block output)
  };

  void build_params() override;
  void finalize() override;
  bool owns_option(const std::string& key) const override { return key == "res2_tail"; }
  void check_forward(int B, int T) const override;
  Ws ws_layout(int B, int T, float* base) const;
  size_t ws_floats(int B, int T) const override { return ws_layout(B, T, nullptr).floats; }
  void forward(const float* feats, int B, int T, float* embed, float* ws, hipStream_t s) override;
};
}  // namespace

Model::Impl* make_res2net(const std::string& arch, int feat_dim, int embed_dim, bool emb_bn, bool two_emb) {
  const Arch* a = std::find_if(std::begin(kArchs), std::end(kArchs), [&](const Arch& k) { return arch == k.name; });
  if (a == std::end(kArchs)) return nullptr;
  WSP_CHECK(!emb_bn, "Res2Net has no emb_bn");
  // res2net.py:110 sizes seg_1 for int(feat_dim / 8) frequency rows while stage 4 keeps ceil(feat_dim / 8)
  WSP_CHECK(feat_dim >= 8 && feat_dim % 8 == 0, "Res2Net feat_dim must be a positive multiple of 8");
  WSP_CHECK(embed_dim > 0, "embed_dim must be positive");
  Res2Net* e = new Res2Net(arch, feat_dim, embed_dim, emb_bn, two_emb);
  e->m = a->m;
  std::copy(std::begin(a->tail), std::end(a->tail), e->tail_stage);
  return e;
}

// state_dict order of Res2Net (320 entries; + 5 with two_emb_layer)
void Res2Net::build_params() {
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
      b.width = planes / 2;
      b.stride = (li > 0 && bi == 0) ? 2 : 1;
      b.out_planes = planes * kExpansion;
      b.has_sc = b.stride != 1 || in_planes != b.out_planes;
      const std::string& p = b.name;
      const int w = b.width;
      add(p + ".conv1.weight", {2 * w, in_planes, 1, 1});
      add_bn(p + ".bn1", 2 * w);
      add(p + ".convs.0.weight", {w, w, 3, 3});
      add_bn(p + ".bns.0", w);
      add(p + ".conv3.weight", {b.out_planes, 2 * w, 1, 1});
      add_bn(p + ".bn3", b.out_planes);
      if (b.has_sc) {
        add(p + ".shortcut.0.weight", {b.out_planes, in_planes, 1, 1});
        add_bn(p + ".shortcut.1", b.out_planes);
      }
      blocks.push_back(b);
      in_planes = b.out_planes;
    }
  }
  const int stats_dim = (feat_dim / 8) * m * 8 * kExpansion;
  add("seg_1.weight", {embed_dim, stats_dim * 2});
  add("seg_1.bias", {embed_dim});
  if (two_emb) {  // res2net.py:142-144: BatchNorm1d(affine=False) + seg_2
    add("seg_bn_1.running_mean", {embed_dim});
    add("seg_bn_1.running_var", {embed_dim});
    add("seg_bn_1.num_batches_tracked", {});
    add("seg_2.weight", {embed_dim, embed_dim});
    add("seg_2.bias", {embed_dim});
  }
}

void Res2Net::finalize() {
  const Folded stem = fold_bn("conv1.weight", "bn1");  // as the ResNets'
  stem_w = dev.upload(stem.w);
  stem_b = dev.upload(stem.b);
  for (Block& b : blocks) {
    const std::string& p = b.name;
    const int w = b.width;
    WSP_CHECK(eres_conv3x3_supported(w) && res2_tail_supported(w), "Res2Net: no kernel for width " + std::to_string(w));
    b.c1 = fold_pw(*this, p + ".conv1.weight", p + ".bn1", 2 * w, b.in_planes, 1);
    b.c2 = fold_pw(*this, p + ".convs.0.weight", p + ".bns.0", w, w, 9);
    b.c3 = fold_pw(*this, p + ".conv3.weight", p + ".bn3", b.out_planes, 2 * w, 1);
    b.c3t = fold_pw(*this, p + ".conv3.weight", p + ".bn3", b.out_planes, 2 * w, 1, true);
    if (b.has_sc) b.sc = fold_pw(*this, p + ".shortcut.0.weight", p + ".shortcut.1", b.out_planes, b.in_planes, 1);
  }
  // seg_1 over TSTP stats; reference flatten index s*C*F4 + c*F4 + f, ours f*2C + s*C + c
  const int C4 = m * kExpansion * 8, F4 = feat_dim / 8;
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

void Res2Net::check_forward(int, int T) const {
  // as every family off the f32 GEMM path: the message names the first of them
  WSP_CHECK(opt.precision == 1, "ResNet runs on the bf16x3 kernels only (precision=1)");
  WSP_CHECK((T + 7) / 8 >= 2, "Res2Net needs >= 9 frames (2 after the three stride-2 stages)");
}

Res2Net::Ws Res2Net::ws_layout(int B, int T, float* base) const {
  // floats per utterance
  size_t big = 0, y = 0, sc = 0;
  int Fi = feat_dim, Ti = T;
  big = (size_t)Fi * Ti * m;
  for (const Block& b : blocks) {
    Fi = (Fi - 1) / b.stride + 1;
    Ti = (Ti - 1) / b.stride + 1;
    const size_t pos = (size_t)Fi * Ti;
    big = std::max(big, pos * b.out_planes);
    y = std::max(y, pos * b.width * 2);
    if (b.has_sc) sc = std::max(sc, pos * b.out_planes);
  }
  const size_t C4 = (size_t)m * kExpansion * 8, K = (size_t)Fi * 2 * C4;
  WsCursor c{base};
  Ws w;
  w.bc = chunk_for(B, std::max(big, std::max(y, sc)) * sizeof(float));
  const size_t bc = w.bc;
  w.X = c.take(bc * big);
  w.O = c.take(bc * big);
  w.Y1 = c.take(bc * y);
  w.S = c.take(bc * y / 2);  // the 3x3 conv's output (unfused schedule)
  w.SC = c.take(bc * sc);
  w.pooled = c.take(bc * K);
  w.E1 = c.take(bc * embed_dim);
  w.scratch_floats = small_linear_scratch_floats((int)bc, embed_dim, (int)K);
  w.scratch = c.take(w.scratch_floats);
  w.floats = c.off;
  return w;
}

void Res2Net::forward(const float* feats, int B, int T, float* embed, float* ws, hipStream_t s) {
  const Ws W = ws_layout(B, T, ws);
  const int bc = W.bc;
  auto pw = [&](const std::string& tag, const Pw& w, const float* in, int lda, const float* in2, int lda2, int ksplit, int nb,
                int Fi, int Ti, int stride, float* out, const float* res, int act) {
    const EresConvArgs a{in, lda, in2, lda2, nb, Fi, Ti, w.K, stride, w.w, w.b, w.N, res, res ? w.N : 0, out, w.N, act,
                         ksplit};
    const double pos = (double)nb * ((Fi - 1) / stride + 1) * ((Ti - 1) / stride + 1);
    run(tag.c_str(), 2.0 * pos * w.N * w.K, s, [&] { launch_eres_pw(a, s); });
  };
  for (int b0 = 0; b0 < B; b0 += bc) {
    const int nb = std::min(bc, B - b0);
    int Fi = feat_dim, Ti = T, Ci = m;
    run("stem", 0, s,
        [&] { launch_resnet_stem(feats + (size_t)b0 * T * feat_dim, nb, T, feat_dim, m, stem_w, stem_b, W.X, s); });
    float* x = W.X;
    float* o = W.O;
    for (const Block& b : blocks) {
      const int Fo = (Fi - 1) / b.stride + 1, To = (Ti - 1) / b.stride + 1;
      const int M = nb * Fo * To, w = b.width;
      const float* res = x;
      const std::string L = ".L" + std::to_string(b.li + 1);  // the profile classes carry the stage
      if (b.has_sc) {
        pw("res2_pw.sc" + L, b.sc, x, Ci, nullptr, 0, 0, nb, Fi, Ti, b.stride, W.SC, nullptr, kEresNone);
        res = W.SC;
      }
      pw("res2_pw.c1" + L, b.c1, x, Ci, nullptr, 0, 0, nb, Fi, Ti, b.stride, W.Y1, nullptr, kEresClamp);
      if (opt.res2_tail == 2 || (opt.res2_tail == 1 && tail_stage[b.li])) {
        const Res2TailArgs a{W.Y1, 2 * w, nb, Fo, To, w, b.c2.w, b.c2.b, b.c3t.w, b.c3t.b, b.out_planes,
                             res, b.out_planes, o, b.out_planes};
        run(("res2_tail" + L).c_str(), 2.0 * M * (9.0 * w * w + 2.0 * w * b.out_planes), s, [&] { launch_res2_tail(a, s); });
      } else {
        const EresConvArgs a{W.Y1, 2 * w, nullptr, 0, nb, Fo, To, w, 1, b.c2.w, b.c2.b, w, nullptr, 0, W.S, w, kEresClamp};
        run(("res2_conv3x3" + L).c_str(), 2.0 * M * w * 9.0 * w, s, [&] { launch_eres_conv3x3(a, s); });
        // conv3 over [S | Y1[:, w:]]
        pw("res2_pw.c3" + L, b.c3, W.S, w, W.Y1 + w, 2 * w, w, nb, Fo, To, 1, o, res, kEresClamp);
      }
      std::swap(x, o);
      Fi = Fo;
      Ti = To;
      Ci = b.out_planes;
    }
    // TSTP over frames of layer4's output for every (utterance, freq) row block, then seg_1 (+ seg_2)
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
