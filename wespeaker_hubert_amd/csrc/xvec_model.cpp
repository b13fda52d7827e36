// x-vector TDNN (tdnn.py XVEC) with TSTP or XI pooling: parameter table, packing, workspace and
// the forward schedule.  Channels-last frames [rows][C].
//
//   frame_1..5  Conv1d with bias and NO padding (k5 d1, k3 d2, k3 d3, k1, k1; F -> 512 -> 512 -> 512
//               -> 512 -> 1500) -> ReLU -> BatchNorm(affine=False): the shared implicit GEMM, the BN
//               as the epilogue's scale / shift.  An utterance of T frames keeps T - 4, T - 8, T - 14
//               rows after frames 1, 2, 3: output rows and input rows differ, so every launch carries
//               T != Ti (uniform batches) or the seg / iseg pair (ragged batches), as the HuBERT CNN.
//   1500        is no multiple of the GEMM's column tile: frame_5 is packed 1536 wide with zero
//               weights, zero bias and a zero shift in the pad columns, which therefore hold exact
//               zeros; pool.lin1's K and pool.lin2's N are padded the same way.  TSTP, XI and seg_1
//               read columns [0, 1500) only.
//   TSTP        launch_frame_stats -> [B][3000]           XI   lin1 (ReLU -> BN) -> lin2 -> launch_xi_pool
//   head        seg_1 -> ReLU -> seg_bn_1 (no affine, folded into seg_2) -> seg_2 = embed_b
#include "model_impl.h"
#include "xi_pool.h"

namespace wsp {

namespace {
constexpr int kHid = 512, kStats = 1500, kStatsP = 1536, kXiHid = 256;
constexpr int kShrink[3] = {4, 8, 14};  // frames an utterance has lost after frame_1, frame_2, frame_3

struct Xvec final : Model::Impl {
  using Impl::Impl;
  bool xi = false;
  ConvW frame[5], lin1, lin2;
  float *prior_mean = nullptr, *prior_logprec = nullptr;
  LinW seg1, seg2;
  struct Ws {
    float *a, *b, *x5, *h, *z, *pooled, *e1;
    int* segs;  // [3][B + 1] row offsets after frames 1, 2, 3 (ragged batches)
    size_t floats;
  };

  int need_frames() const { return xi ? 15 : 16; }  // T' = T - 14 >= 1; TSTP's unbiased variance needs 2
  int pooled_dim() const { return xi ? kStats : 2 * kStats; }
  void build_params() override;
  ConvW pack_tdnn(const std::string& p, int N, int Np, int cin, int taps);
  void finalize() override;
  void check_forward(int B, int T) const override;
  Ws ws_layout(size_t B, size_t M, float* base) const;
  int chunk(int B, int T) const { return chunk_for(B, (size_t)T * kStatsP * sizeof(float)); }
  size_t ws_floats(int B, int T) const override {
    const size_t bc = chunk(B, T);
    return ws_layout(bc, bc * T, nullptr).floats;
  }
  void forward(const float* feats, int B, int T, float* embed, float* ws, hipStream_t s) override;
  bool has_segments() const override { return true; }
  size_t ws_floats_segments(int B, int M) const override { return ws_layout(B, M, nullptr).floats; }
  void forward_segments(const float* feats, int B, const int* seg, int M, float* embed, float* ws,
                        hipStream_t s) override;
  void forward_chunk(const float* feats, int B, int T, float* embed, float* ws, hipStream_t s, const int* seg, int M_seg);
};
}  // namespace

Model::Impl* make_xvec(const std::string& arch, int feat_dim, int embed_dim, bool emb_bn, bool two_emb) {
  if (arch != "XVEC" && arch != "XI_VEC_XVEC") return nullptr;
  WSP_CHECK(!emb_bn, "XVEC has no emb_bn");
  WSP_CHECK(!two_emb, "XVEC has no two_emb_layer (seg_2 is always there: the embedding is embed_b)");
  WSP_CHECK(feat_dim > 0 && feat_dim % 4 == 0, "XVEC feat_dim must be a positive multiple of 4");
  WSP_CHECK(embed_dim > 0, "embed_dim must be positive");
  Xvec* m = new Xvec(arch, feat_dim, embed_dim, emb_bn, two_emb);
  m->xi = arch == "XI_VEC_XVEC";  // the C ABI has no pooling argument: the arch string carries it
  m->opt.x3_variant = 7;
  return m;
}

// state_dict order: 32 entries with TSTP, 43 with XI
void Xvec::build_params() {
  const int64_t cin[5] = {feat_dim, kHid, kHid, kHid, kHid}, cout[5] = {kHid, kHid, kHid, kHid, kStats};
  const int64_t taps[5] = {5, 3, 3, 1, 1};
  for (int i = 0; i < 5; ++i) {
    const std::string p = "frame_" + std::to_string(i + 1);
    add(p + ".conv_1d.weight", {cout[i], cin[i], taps[i]});
    add(p + ".conv_1d.bias", {cout[i]});
    add(p + ".bn.running_mean", {cout[i]});
    add(p + ".bn.running_var", {cout[i]});
    add(p + ".bn.num_batches_tracked", {});
  }
  if (xi) {
    add("pool.prior_mean", {1, kStats});
    add("pool.prior_logprec", {1, kStats});
    add("pool.lin1_relu_bn.0.weight", {kXiHid, kStats, 1});
    add("pool.lin1_relu_bn.0.bias", {kXiHid});
    add_bn("pool.lin1_relu_bn.2", kXiHid);
    add("pool.lin2.weight", {kStats, kXiHid, 1});
    add("pool.lin2.bias", {kStats});
  }
  add("seg_1.weight", {embed_dim, pooled_dim()});
  add("seg_1.bias", {embed_dim});
  add("seg_bn_1.running_mean", {embed_dim});
  add("seg_bn_1.running_var", {embed_dim});
  add("seg_bn_1.num_batches_tracked", {});
  add("seg_2.weight", {embed_dim, embed_dim});
  add("seg_2.bias", {embed_dim});
}

// frame_k: conv [N][cin][taps] packed Np >= N wide; BatchNorm(affine=False) behind the ReLU as the
// epilogue's scale / shift.  Pad columns: zero weights, bias and shift -> exact zeros.
ConvW Xvec::pack_tdnn(const std::string& p, int N, int Np, int cin, int taps) {
  const size_t K = (size_t)cin * taps;
  std::vector<float> w(Np * K, 0.f), b(Np, 0.f), sc(Np, 1.f), sh(Np, 0.f);
  const auto& W = P(p + ".conv_1d.weight");
  const auto& bb = P(p + ".conv_1d.bias");
  const auto& rm = P(p + ".bn.running_mean");
  const auto& rv = P(p + ".bn.running_var");
  std::copy(W.begin(), W.end(), w.begin());
  for (int n = 0; n < N; ++n) {
    const double s = 1.0 / std::sqrt((double)rv[n] + kBnEps);
    b[n] = bb[n];
    sc[n] = (float)s;
    sh[n] = (float)(-(double)rm[n] * s);
  }
  ConvW cw = pack_conv(w, Np, cin, taps, b.data(), "");
  cw.scale = dev.upload(sc);
  cw.shift = dev.upload(sh);
  return cw;
}

void Xvec::finalize() {
  const int cin[5] = {feat_dim, kHid, kHid, kHid, kHid}, taps[5] = {5, 3, 3, 1, 1};
  for (int i = 0; i < 5; ++i)
    frame[i] = pack_tdnn("frame_" + std::to_string(i + 1), i == 4 ? kStats : kHid, i == 4 ? kStatsP : kHid, cin[i], taps[i]);
  if (xi) {
    // lin1 reads the 1536-wide frame_5 output: its K is padded with zero columns
    const auto& W1 = P("pool.lin1_relu_bn.0.weight");
    std::vector<float> w1((size_t)kXiHid * kStatsP, 0.f);
    for (int n = 0; n < kXiHid; ++n) {
      const auto row = W1.begin() + (size_t)n * kStats;
      std::copy(row, row + kStats, w1.begin() + (size_t)n * kStatsP);
    }
    lin1 = pack_conv(w1, kXiHid, kStatsP, 1, P("pool.lin1_relu_bn.0.bias").data(), "pool.lin1_relu_bn.2");
    // lin2's N is padded: logits past column 1500 are zeros nobody reads
    std::vector<float> w2((size_t)kStatsP * kXiHid, 0.f), b2(kStatsP, 0.f);
    const auto& W2 = P("pool.lin2.weight");
    const auto& B2 = P("pool.lin2.bias");
    std::copy(W2.begin(), W2.end(), w2.begin());
    std::copy(B2.begin(), B2.end(), b2.begin());
    lin2 = pack_conv(w2, kStatsP, kXiHid, 1, b2.data(), "");
    prior_mean = dev.upload(P("pool.prior_mean"));
    prior_logprec = dev.upload(P("pool.prior_logprec"));
  }
  const int K = pooled_dim(), D = embed_dim;
  seg1 = pack_lin(P("seg_1.weight").data(), D, K, K, P("seg_1.bias").data());
  // seg_2(BN(relu(embed_a))), BN without affine: (W2 diag(s)) r + (b2 - W2 (rm s))
  const auto& rm = P("seg_bn_1.running_mean");
  const auto& rv = P("seg_bn_1.running_var");
  const auto& W2 = P("seg_2.weight");
  const auto& b2 = P("seg_2.bias");
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

void Xvec::check_forward(int, int T) const {
  WSP_CHECK(opt.precision == 1, "XVEC runs on the bf16x3 kernels only (precision=1)");
  if (xi)
    WSP_CHECK(T >= 15, "XI_VEC_XVEC needs >= 15 frames (the unpadded convs keep T - 14)");
  else
    WSP_CHECK(T >= 16, "XVEC needs >= 16 frames (the unpadded convs keep T - 14, TSTP's variance needs 2)");
}

// M = input frame rows of the (sub-)batch; every later tensor has fewer rows
Xvec::Ws Xvec::ws_layout(size_t B, size_t M, float* base) const {
  WsCursor c{base};
  Ws w;
  w.a = c.take(M * kHid);
  w.b = c.take(M * kHid);
  w.x5 = c.take(M * kStatsP);
  w.h = xi ? c.take(M * kXiHid) : nullptr;
  w.z = xi ? c.take(M * kStatsP) : nullptr;
  w.pooled = c.take(B * 2 * kStatsP);
  w.e1 = c.take(B * embed_dim);
  w.segs = reinterpret_cast<int*>(c.take(3 * (B + 1)));
  w.floats = c.off;
  return w;
}

void Xvec::forward(const float* feats, int B, int T, float* embed, float* ws, hipStream_t s) {
  const int bc = chunk(B, T);
  for (int c0 = 0; c0 < B; c0 += bc)
    forward_chunk(feats + (size_t)c0 * T * feat_dim, std::min(bc, B - c0), T, embed + (size_t)c0 * embed_dim, ws, s,
                  nullptr, 0);
}

void Xvec::forward_segments(const float* feats, int B, const int* seg, int M, float* embed, float* ws, hipStream_t s) {
  WSP_CHECK(opt.precision == 1, "XVEC runs on the bf16x3 kernels only (precision=1)");
  // the offsets live on the device: only their total can be checked here; the caller guarantees the
  // per-utterance minimum (wespeaker_amd.h), as the Python host does before it calls
  WSP_CHECK((long long)M >= (long long)B * need_frames(),
            arch + " needs >= " + std::to_string(need_frames()) + " frames per utterance");
  forward_chunk(feats, B, 1, embed, ws, s, seg, M);
}

void Xvec::forward_chunk(const float* feats, int B, int T, float* embed, float* ws, hipStream_t s, const int* seg,
                         int M_seg) {
  const Ws W = ws_layout(B, seg ? M_seg : (size_t)B * T, ws);
  // rows and per-utterance tables of the four tensor lengths: the input, after frames 1, 2, 3
  int rows[4], len[4];
  const int* tab[4] = {seg, nullptr, nullptr, nullptr};
  rows[0] = seg ? M_seg : B * T;
  len[0] = T;
  for (int k = 0; k < 3; ++k) {
    rows[k + 1] = rows[0] - B * kShrink[k];
    len[k + 1] = T - kShrink[k];
    if (seg) tab[k + 1] = W.segs + (size_t)k * (B + 1);
  }
  if (seg) run("seg_tables", 0, s, [&] { launch_valid_conv_offsets(seg, B, kShrink, 3, W.segs, s); });
  // level li tensor -> level lo tensor (lo == li: a 1x1 conv)
  auto tdnn = [&](const char* tag, const ConvW& cw, const float* a, int lda, float* out, int ldo, int dil, int li,
                  int lo, int act) {
    ConvGemmArgs g{};
    one_operand(g, a, lda, cw.cin);
    fill(g, cw, rows[lo], seg ? 1 : len[lo], dil, 0, out, ldo, act, nullptr, true, tab[lo], B);
    if (li != lo) {
      g.Ti = seg ? rows[li] : len[li];
      g.iseg = tab[li];
    }
    run(tag, 2.0 * rows[lo] * cw.N * cw.K, s, [&] { launch(g, cw, s); });
  };
  tdnn("tdnn_k5", frame[0], feats, feat_dim, W.a, kHid, 1, 0, 1, kActRelu);
  tdnn("tdnn_k3", frame[1], W.a, kHid, W.b, kHid, 2, 1, 2, kActRelu);
  tdnn("tdnn_k3", frame[2], W.b, kHid, W.a, kHid, 3, 2, 3, kActRelu);
  tdnn("tdnn_1x1", frame[3], W.a, kHid, W.b, kHid, 1, 3, 3, kActRelu);
  tdnn("tdnn_1x1", frame[4], W.b, kHid, W.x5, kStatsP, 1, 3, 3, kActRelu);
  const int T3 = len[3];
  const int* seg3 = tab[3];
  const int K = pooled_dim();
  if (xi) {
    tdnn("xi_lin1", lin1, W.x5, kStatsP, W.h, kXiHid, 1, 3, 3, kActRelu);
    tdnn("xi_lin2", lin2, W.h, kXiHid, W.z, kStatsP, 1, 3, 3, kActNone);
    const XiPoolArgs a{W.z, kStatsP, W.x5, kStatsP, prior_mean, prior_logprec, B, T3, kStats, seg3, W.pooled, kStatsP};
    run("xi_pool", 0, s, [&] { launch_xi_pool(a, s); });
  } else {
    run("tstp", 0, s, [&] { launch_frame_stats(W.x5, kStatsP, B, T3, kStats, W.pooled, 2 * kStatsP, 1, kStats, s, seg3); });
  }
  run("head", 0, s, [&] {
    launch_small_linear({W.pooled, xi ? kStatsP : 2 * kStatsP, seg1.wt, seg1.bias, W.e1, embed_dim, B, K, embed_dim, 1}, s);
    launch_small_linear({W.e1, embed_dim, seg2.wt, seg2.bias, embed, embed_dim, B, embed_dim, embed_dim, 0}, s);
  });
}

}  // namespace wsp
