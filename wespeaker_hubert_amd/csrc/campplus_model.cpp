// CAM++ (campplus.py:333-413): parameter table, BatchNorm folds / packing, workspace and the
// forward schedule.  FCM head in NHWC [B][F][T][32] (stem and stride-1 3x3 convs on the ResNet
// kernels, the frequency-strided convs on fcm_conv.hip), then channels-last frame rows: the
// strided TDNN on the implicit GEMM, the three dense blocks on cam_dense.hip — each block one
// buffer [B T'][Cmax] that its layers append 32 columns to in place — TSTP and the embedding.
#include "cam_dense.h"
#include "conv3x3_img.h"
#include "fcm_conv.h"
#include "model_impl.h"

namespace wsp {

namespace {
constexpr int kCamLayers[3] = {12, 24, 16}, kCamDil[3] = {1, 2, 2};
constexpr int kCamC0[3] = {128, 256, 512}, kCamCmax[3] = {512, 1024, 1024};
const char* const kFcmBlocks[4] = {"head.layer1.0", "head.layer1.1", "head.layer2.0", "head.layer2.1"};

std::string cam_layer_name(int bi, int li) {
  return "xvector.block" + std::to_string(bi + 1) + ".tdnnd" + std::to_string(li + 1);
}

// FCM head NHWC [B][F][T][32], then frame rows [B][T'][C]
struct Campplus final : Model::Impl {
  using Impl::Impl;
  float *stem_w = nullptr, *stem_b = nullptr;  // head.conv1 + bn1
  struct FcmBlock {
    bool strided = false;  // first block of a stage: conv1 and the projection shortcut stride (2, 1)
    // BN-folded weights and biases: conv1 as fcm_conv.hip fragments when strided, else as
    // conv3x3_img.hip fragments like conv2; the shortcut as fcm_conv.hip fragments
    void *w1 = nullptr, *w2 = nullptr, *wsc = nullptr;
    float *b1 = nullptr, *b2 = nullptr, *bsc = nullptr;
  } fcm_blk[4];
  void* fcm_out_w = nullptr;  // head.conv2 + bn2
  float* fcm_out_b = nullptr;
  ConvW cam_tdnn;
  struct CamLayer {
    int cin = 0;
    float *s1 = nullptr, *t1 = nullptr, *s2 = nullptr, *t2 = nullptr;  // nonlinear1 / nonlinear2 as affines
    void *w1 = nullptr, *wl = nullptr;  // linear1 / linear_local as cam_pack_b fragments
    LinW l1, l2;                        // the context mask's two linears
  };
  struct CamBlock {
    std::vector<CamLayer> layers;
    float *ts = nullptr, *tt = nullptr;  // transit BatchNorm
    void* tw = nullptr;
  } cam_blk[3];
  float *cam_out_s = nullptr, *cam_out_t = nullptr;  // out_nonlinear
  LinW cam_head;  // dense with its affine-free BatchNorm folded in
  struct Ws {
    float *X, *O, *Y1, *SC;         // FCM: [F][T][32] and [F/2][T][32] per utterance
    float *D[3], *H, *Z, *S;        // dense buffers [M'][Cmax], h [M'][128], transit 3 [M'][512], unfused scratch
    float *segsum, *mask, *pooled;  // [B][nseg][128], [B][nseg][32], [B][1024]
    size_t floats;
    int bc;  // utterances per forward chunk: the widest operand is the stem's output or a 1024-wide dense buffer
  };

  void build_params() override;
  void finalize() override;
  void check_forward(int B, int T) const override;
  Ws ws_layout(int B, int T, float* base) const;
  size_t ws_floats(int B, int T) const override { return ws_layout(B, T, nullptr).floats; }
  void forward(const float* feats, int B, int T, float* embed, float* ws, hipStream_t s) override;
};
}  // namespace

Model::Impl* make_campplus(const std::string& arch, int feat_dim, int embed_dim, bool emb_bn, bool two_emb) {
  // campplus.py:333-413: FCM head + dense TDNN, TSTP, embedding without an affine BatchNorm tail
  if (arch != "CAMPPlus") return nullptr;
  WSP_CHECK(!two_emb && !emb_bn, "CAMPPlus has no emb_bn / two_emb_layer");
  WSP_CHECK(feat_dim >= 8 && feat_dim % 8 == 0, "CAMPPlus feat_dim must be a positive multiple of 8");
  WSP_CHECK(embed_dim > 0, "embed_dim must be positive");
  Campplus* m = new Campplus(arch, feat_dim, embed_dim, emb_bn, two_emb);
  m->opt.x3_variant = 4;  // xvector.tdnn is the one implicit GEMM (N = 128)
  return m;
}

// state_dict order of CAMPPlus(feat_dim, embed_dim) (937 entries)
void Campplus::build_params() {
  add("head.conv1.weight", {32, 1, 3, 3});
  add_bn("head.bn1", 32);
  for (int i = 0; i < 4; ++i) {
    const std::string p = kFcmBlocks[i];
    add(p + ".conv1.weight", {32, 32, 3, 3});
    add_bn(p + ".bn1", 32);
    add(p + ".conv2.weight", {32, 32, 3, 3});
    add_bn(p + ".bn2", 32);
    if (i % 2 == 0) {
      add(p + ".shortcut.0.weight", {32, 32, 1, 1});
      add_bn(p + ".shortcut.1", 32);
    }
  }
  add("head.conv2.weight", {32, 32, 3, 3});
  add_bn("head.bn2", 32);
  add("xvector.tdnn.linear.weight", {128, 32 * (feat_dim / 8), 5});
  add_bn("xvector.tdnn.nonlinear.batchnorm", 128);
  for (int bi = 0; bi < 3; ++bi) {
    for (int li = 0; li < kCamLayers[bi]; ++li) {
      const std::string p = cam_layer_name(bi, li);
      const int cin = kCamC0[bi] + 32 * li;
      add_bn(p + ".nonlinear1.batchnorm", cin);
      add(p + ".linear1.weight", {128, cin, 1});
      add_bn(p + ".nonlinear2.batchnorm", 128);
      add(p + ".cam_layer.linear_local.weight", {32, 128, 3});
      add(p + ".cam_layer.linear1.weight", {64, 128, 1});
      add(p + ".cam_layer.linear1.bias", {64});
      add(p + ".cam_layer.linear2.weight", {32, 64, 1});
      add(p + ".cam_layer.linear2.bias", {32});
    }
    const std::string t = "xvector.transit" + std::to_string(bi + 1);
    add_bn(t + ".nonlinear.batchnorm", kCamCmax[bi]);
    add(t + ".linear.weight", {kCamCmax[bi] / 2, kCamCmax[bi], 1});
  }
  add_bn("xvector.out_nonlinear.batchnorm", 512);
  add("xvector.dense.linear.weight", {embed_dim, 1024, 1});
  add("xvector.dense.nonlinear.batchnorm.running_mean", {embed_dim});
  add("xvector.dense.nonlinear.batchnorm.running_var", {embed_dim});
  add("xvector.dense.nonlinear.batchnorm.num_batches_tracked", {});
}

void Campplus::finalize() {
  auto up_affine = [&](const std::string& bn, float*& sc, float*& sh) {
    std::vector<double> a, b;
    bn_affine(bn, a, b);
    sc = dev.upload(std::vector<float>(a.begin(), a.end()));
    sh = dev.upload(std::vector<float>(b.begin(), b.end()));
  };
  auto up_frag = [&](const std::vector<float>& w, int N, int K) { return dev.upload_u16(cam_pack_b(w.data(), N, K, K)); };
  // 32 -> 32 conv with its BatchNorm folded in, k = tap * 32 + c: the fragments of fcm_conv.hip
  // (cam_pack_b) or, img, of conv3x3_img.hip (pack_frag), and the bias
  WSP_CHECK(conv3x3_img_supported(32), "CAMPPlus: the 32-channel 3x3 image kernel is missing");
  auto fold_frag = [&](const std::string& wname, const std::string& bn, int taps, bool img, void*& frag,
                       float*& bias) {
    const Folded f = fold_bn(wname, bn);
    const int K = 32 * taps;
    const std::vector<float> wk = pack::conv_kmajor(f.w, 32, 32, taps, K);
    frag = img ? pack_frag(wk, 32, K) : up_frag(wk, 32, K);
    bias = dev.upload(f.b);
  };
  const Folded stem = fold_bn("head.conv1.weight", "head.bn1");  // as the ResNets'
  stem_w = dev.upload(stem.w);
  stem_b = dev.upload(stem.b);
  for (int i = 0; i < 4; ++i) {
    const std::string p = kFcmBlocks[i];
    FcmBlock& fb = fcm_blk[i];
    fb.strided = i % 2 == 0;
    fold_frag(p + ".conv1.weight", p + ".bn1", 9, !fb.strided, fb.w1, fb.b1);
    fold_frag(p + ".conv2.weight", p + ".bn2", 9, true, fb.w2, fb.b2);
    if (fb.strided) fold_frag(p + ".shortcut.0.weight", p + ".shortcut.1", 1, false, fb.wsc, fb.bsc);
  }
  fold_frag("head.conv2.weight", "head.bn2", 9, false, fcm_out_w, fcm_out_b);
  {
    // xvector.tdnn: the reference's input channel c * F8 + f (FCM.forward's reshape) is our
    // frame-row column f * 32 + c
    const int F8 = feat_dim / 8, CF = 32 * F8;
    const Folded t = fold_bn("xvector.tdnn.linear.weight", "xvector.tdnn.nonlinear.batchnorm");
    std::vector<float> wp(t.w.size());
    for (int n = 0; n < 128; ++n)
      for (int f = 0; f < F8; ++f)
        for (int c = 0; c < 32; ++c)
          for (int j = 0; j < 5; ++j)
            wp[((size_t)n * CF + f * 32 + c) * 5 + j] = t.w[((size_t)n * CF + c * F8 + f) * 5 + j];
    cam_tdnn = pack_conv(wp, 128, CF, 5, t.b.data(), "");
  }
  for (int bi = 0; bi < 3; ++bi) {
    CamBlock& cb = cam_blk[bi];
    cb.layers.resize(kCamLayers[bi]);
    for (int li = 0; li < kCamLayers[bi]; ++li) {
      const std::string p = cam_layer_name(bi, li);
      CamLayer& L = cb.layers[li];
      L.cin = kCamC0[bi] + 32 * li;
      up_affine(p + ".nonlinear1.batchnorm", L.s1, L.t1);
      L.w1 = up_frag(P(p + ".linear1.weight"), 128, L.cin);
      up_affine(p + ".nonlinear2.batchnorm", L.s2, L.t2);
      L.wl = up_frag(pack::conv_kmajor(P(p + ".cam_layer.linear_local.weight"), 32, 128, 3, 384), 32, 384);
      L.l1 = pack_lin(P(p + ".cam_layer.linear1.weight").data(), 64, 128, 128, P(p + ".cam_layer.linear1.bias").data());
      L.l2 = pack_lin(P(p + ".cam_layer.linear2.weight").data(), 32, 64, 64, P(p + ".cam_layer.linear2.bias").data());
    }
    const std::string t = "xvector.transit" + std::to_string(bi + 1);
    up_affine(t + ".nonlinear.batchnorm", cb.ts, cb.tt);
    cb.tw = up_frag(P(t + ".linear.weight"), kCamCmax[bi] / 2, kCamCmax[bi]);
  }
  up_affine("xvector.out_nonlinear.batchnorm", cam_out_s, cam_out_t);
  {
    // dense + BatchNorm1d(affine=False): (W x - rm) / sqrt(rv + eps) = (W s) x - rm s
    const auto& W = P("xvector.dense.linear.weight");
    const auto& rm = P("xvector.dense.nonlinear.batchnorm.running_mean");
    const auto& rv = P("xvector.dense.nonlinear.batchnorm.running_var");
    std::vector<float> w((size_t)embed_dim * 1024), b(embed_dim);
    for (int n = 0; n < embed_dim; ++n) {
      const double sn = 1.0 / std::sqrt((double)rv[n] + kBnEps);
      for (int k = 0; k < 1024; ++k) w[(size_t)n * 1024 + k] = (float)(W[(size_t)n * 1024 + k] * sn);
      b[n] = (float)(-(double)rm[n] * sn);
    }
    cam_head = pack_lin(w.data(), embed_dim, 1024, 1024, b.data());
  }
}

void Campplus::check_forward(int, int T) const {
  // as every family off the f32 GEMM path: the message names the first of them
  WSP_CHECK(opt.precision == 1, "ResNet runs on the bf16x3 kernels only (precision=1)");
  WSP_CHECK(T >= 3, "CAMPPlus needs >= 3 frames (2 after the stride-2 TDNN)");
}

Campplus::Ws Campplus::ws_layout(int B, int T, float* base) const {
  const size_t Tp = (size_t)(T - 1) / 2 + 1, nseg = (Tp + kCamSeg - 1) / kCamSeg, F = feat_dim;
  WsCursor c{base};
  Ws w;
  w.bc = chunk_for(B, std::max(F * T * 32, Tp * 1024) * sizeof(float));
  const size_t bc = w.bc, Mp = bc * Tp;
  w.X = c.take(bc * F * T * 32);
  w.O = c.take(bc * F * T * 32);
  w.Y1 = c.take(bc * (F / 2) * T * 32);
  w.SC = c.take(bc * (F / 2) * T * 32);
  for (int i = 0; i < 3; ++i) w.D[i] = c.take(Mp * kCamCmax[i]);
  w.H = c.take(Mp * 128);
  w.Z = c.take(Mp * 512);
  w.S = c.take(Mp * 1024);
  w.segsum = c.take(bc * nseg * 128);
  w.mask = c.take(bc * nseg * 32);
  w.pooled = c.take(bc * 1024);
  w.floats = c.off;
  return w;
}

void Campplus::forward(const float* feats, int B, int T, float* embed, float* ws, hipStream_t s) {
  const Ws W = ws_layout(B, T, ws);
  const int bc = W.bc;
  const int Tp = (T - 1) / 2 + 1;
  static const char* kGemm[3] = {"cam_gemm.b1", "cam_gemm.b2", "cam_gemm.b3"};
  static const char* kLocal[3] = {"cam_local.b1", "cam_local.b2", "cam_local.b3"};
  for (int b0 = 0; b0 < B; b0 += bc) {
    const int nb = std::min(bc, B - b0);
    run("stem", 0, s, [&] {
      launch_resnet_stem(feats + (size_t)b0 * T * feat_dim, nb, T, feat_dim, 32, stem_w, stem_b, W.X, s);
    });
    // ---- FCM: two stages of (strided block, plain block), then conv2
    float* x = W.X;
    float* o = W.O;
    int Fi = feat_dim;
    // stride-1 3x3 conv (+ residual) + ReLU on the image kernel itself: no other path serves it
    auto conv_img = [&](const void* w, const float* bias, const float* in, float* out, int F, const float* res) {
      const Conv3x3Args a{in, out, nb, F, T, w, bias, nullptr, nullptr, res, 1, 0};
      run("fcm_conv3x3", 2.0 * nb * F * T * 32 * 288, s, [&] { launch_conv3x3_img(a, 32, s); });
    };
    for (int i = 0; i < 4; ++i) {
      const FcmBlock& fb = fcm_blk[i];
      const float* res = x;
      int Fo = Fi;
      if (fb.strided) {
        Fo = (Fi - 1) / 2 + 1;
        const FcmConvArgs a{x, W.Y1, nb, Fi, T, fb.w1, fb.b1, 1, 0, fb.wsc, fb.bsc, W.SC};
        run("fcm_strided", 2.0 * nb * Fo * T * 32 * (288 + 32), s, [&] { launch_fcm_conv(a, s); });
        res = W.SC;
      } else {
        conv_img(fb.w1, fb.b1, x, W.Y1, Fi, nullptr);
      }
      conv_img(fb.w2, fb.b2, W.Y1, o, Fo, res);
      std::swap(x, o);
      Fi = Fo;
    }
    const int F8 = (Fi - 1) / 2 + 1, CF = 32 * F8;
    {
      const FcmConvArgs a{x, o, nb, Fi, T, fcm_out_w, fcm_out_b, 1, 1, nullptr, nullptr, nullptr};
      run("fcm_strided", 2.0 * nb * F8 * T * 32 * 288, s, [&] { launch_fcm_conv(a, s); });
    }
    const int M = nb * Tp;
    {  // xvector.tdnn: k5, stride 2, pad 2 over the frame rows [nb T][CF] -> D1[:, :128]
      ConvGemmArgs g{};
      one_operand(g, o, CF, CF);
      fill(g, cam_tdnn, M, Tp, 1, 2, W.D[0], kCamCmax[0], kActRelu, nullptr, true, nullptr, 0);
      g.stride = 2;
      g.Ti = T;
      run("cam_tdnn", 2.0 * M * 128 * cam_tdnn.K, s, [&] { launch(g, cam_tdnn, s); });
    }
    // ---- dense blocks
    for (int bi = 0; bi < 3; ++bi) {
      const CamBlock& cb = cam_blk[bi];
      float* D = W.D[bi];
      const int ld = kCamCmax[bi];
      auto gemm_pro = [&](const char* tag, int K, int N, const float* s1, const float* t1, const void* w,
                          const float* s2, const float* t2, float* out, int ldo, float* segsum) {
        CamGemmArgs a{D, ld, M, Tp, K, N, s1, t1, w, s2, t2, out, ldo, segsum};
        if (!opt.cam_fused) {  // A/B option: the BN-ReLU as an elementwise pass of its own
          run("cam_bnrelu", 0, s, [&] { launch_cam_bnrelu(D, ld, M, K, s1, t1, W.S, 1024, s); });
          a.a = W.S;
          a.lda = 1024;
          a.s1 = a.t1 = nullptr;
        }
        run(tag, 2.0 * M * N * K, s, [&] { launch_cam_gemm(a, s); });
      };
      for (const CamLayer& L : cb.layers) {
        gemm_pro(kGemm[bi], L.cin, 128, L.s1, L.t1, L.w1, L.s2, L.t2, W.H, 128, W.segsum);
        run("cam_mask", 0, s,
            [&] { launch_cam_mask(W.segsum, nb, Tp, L.l1.wt, L.l1.bias, L.l2.wt, L.l2.bias, W.mask, s); });
        const CamLocalArgs a{W.H, 128, M, Tp, kCamDil[bi], L.wl, W.mask, D + L.cin, ld};
        run(kLocal[bi], 2.0 * M * 32 * 384, s, [&] { launch_cam_local(a, s); });
      }
      // transit: BN-ReLU on the whole concatenation, 1x1 conv into the next block's buffer;
      // the last one also applies out_nonlinear
      const bool last = bi == 2;
      gemm_pro("cam_transit", ld, ld / 2, cb.ts, cb.tt, cb.tw, last ? cam_out_s : nullptr, last ? cam_out_t : nullptr,
               last ? W.Z : W.D[bi + 1], last ? 512 : kCamCmax[bi + 1], nullptr);
    }
    run("tstp_head", 0, s, [&] {
      launch_frame_stats(W.Z, 512, nb, Tp, 512, W.pooled, 1024, 1, 512, s);
      launch_small_linear({W.pooled, 1024, cam_head.wt, cam_head.bias, embed + (size_t)b0 * embed_dim, embed_dim, nb,
                           1024, embed_dim, 0},
                          s);
    });
  }
}

}  // namespace wsp
