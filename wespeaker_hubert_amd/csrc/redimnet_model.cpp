// ReDimNetB2 (redimnet.py:622-947): parameter table, folds / packing, workspace and the forward
// schedule.  One activation layout throughout: frame rows [B * T][1152], column f * c + ch, which
// is the reference's 1-D view and every stage's 2-D view [B][T][F][c] at once (redimnet.h).  A
// stage is: the softmax-weighted sum of all earlier 1-D outputs feeding the (s, 1) entry conv (one
// launch), its 2-D ConvNeXt blocks (one launch each), then the 1-D block — the 1152 -> hC
// reduction, the hC x hC linears and the hC -> 1152 expansion (+ skip in its epilogue) on the
// shared implicit GEMM, the four depthwise ConvNeXt blocks (one launch each), streaming attention
// and the row LayerNorms on redimnet.hip.  The hC-wide tensors are 4 .. 12 times narrower than the
// activation, so their extra passes are cheap.  GEMM output widths are padded to a multiple of 64
// with zero weight rows (hC = 96 / 144 / 288 -> 128 / 192 / 320), which both GEMM paths take.  The
// head is ECAPA's GLOB ASTP at 1152 channels and seg_1 (+ seg_2).
#include "model_impl.h"
#include "redimnet.h"

namespace wsp {

namespace {
constexpr int kC0 = 16, kF0 = 72, kD = kRdWidth, kHeads = 4, kStages = 6;
constexpr int kStride[kStages] = {1, 2, 1, 2, 1, 2};
constexpr int kBlocks[kStages] = {2, 2, 3, 4, 4, 4};
constexpr int kRed[kStages] = {12, 12, 12, 8, 8, 4};
constexpr int kDwK[4] = {7, 19, 31, 59};
constexpr double kLnEps = 1e-6;

struct Redimnet final : Model::Impl {
  using Impl::Impl;
  struct Pw {  // depthwise / grouped taps with the BatchNorm folded in, and the k-major 1x1 conv
    float *wd = nullptr, *bd = nullptr, *wp = nullptr, *bp = nullptr;
  };
  struct Stage {
    int cin = 0, c = 0, F = 0, s = 1, hC = 0, hCp = 0, qkvp = 0;
    float *ew = nullptr, *eb = nullptr;  // entry conv, k-major [s*cin][c]
    std::vector<Pw> b2;
    ConvW red, qkv, outp, ff1, ff2, exp;
    float *ln0_g = nullptr, *ln0_b = nullptr, *ln1_g = nullptr, *ln1_b = nullptr, *ln2_g = nullptr, *ln2_b = nullptr;
    Pw b1[4];
  };
  Stage st[kStages];
  float* sw[kStages + 1] = {};  // softmax of inputs_weights[i] over its inputs axis, [i + 1][1152]
  float *stem_w = nullptr, *stem_b = nullptr, *stem_g = nullptr, *stem_beta = nullptr;
  ConvW pool1, pool2;
  LinW pool1_ctx, seg1, seg2;
  struct Ws {
    float *O[kStages + 1], *P[2], *h[2], *qkv, *att, *tmp, *patt, *gstats, *rowb, *pooled, *E1, *scratch;
    size_t scratch_floats, floats;
    int bc;
  };

  void build_params() override;
  std::vector<float> kmajor(const std::vector<float>& w, int N, int K) const;
  ConvW lin(const std::vector<float>& w, const std::vector<float>& b, int N, int K);
  Pw fold_dw(const std::string& p, int C, int gin, int taps);
  void finalize() override;
  int min_frames() const override { return 2; }  // ASTP's context std is the unbiased one
  Ws ws_layout(int B, int T, float* base) const;
  size_t ws_floats(int B, int T) const override { return ws_layout(B, T, nullptr).floats; }
  void forward(const float* feats, int B, int T, float* embed, float* ws, hipStream_t s) override;
};
}  // namespace

Model::Impl* make_redimnet(const std::string& arch, int feat_dim, int embed_dim, bool emb_bn, bool two_emb) {
  if (arch != "ReDimNetB2") return nullptr;  // B0 / B1 / B3..B6: other block types, group sizes, a stride-3 stage
  WSP_CHECK(!emb_bn, "ReDimNetB2 has no emb_bn");
  WSP_CHECK(feat_dim == kF0, "ReDimNetB2 path implements feat_dim 72 (C * F = 1152)");
  WSP_CHECK(embed_dim > 0, "embed_dim must be positive");
  return new Redimnet(arch, feat_dim, embed_dim, emb_bn, two_emb);
}

// state_dict order: 548 entries (+ 5 with two_emb_layer)
void Redimnet::build_params() {
  add("backbone.inputs_weights.0", {1, 1, 1, 1});
  for (int i = 1; i <= kStages; ++i) add("backbone.inputs_weights." + std::to_string(i), {1, i + 1, kD, 1});
  add("backbone.stem.0.weight", {kC0, 1, 3, 3});
  add("backbone.stem.0.bias", {kC0});
  add("backbone.stem.1.weight", {kC0});
  add("backbone.stem.1.bias", {kC0});
  int c = kC0, F = kF0;
  for (int si = 0; si < kStages; ++si) {
    Stage& g = st[si];
    g.cin = c;
    g.s = kStride[si];
    g.c = c = c * g.s;
    g.F = F = F / g.s;
    g.hC = kD / kRed[si];
    g.hCp = round_up(g.hC, 64);
    g.qkvp = round_up(3 * g.hC, 64);
    g.b2.assign(kBlocks[si], Pw{});
    const std::string p = "backbone.stage" + std::to_string(si);
    add(p + ".0.weight", {g.c, g.cin, g.s, 1});
    add(p + ".0.bias", {g.c});
    for (int bi = 1; bi <= kBlocks[si]; ++bi) {
      const std::string q = p + "." + std::to_string(bi) + ".conv_block";
      add(q + ".dwconvs.0.weight", {g.c, 4, 3, 3});
      add(q + ".dwconvs.0.bias", {g.c});
      add_bn(q + ".norm", g.c);
      add(q + ".pwconv1.weight", {g.c, g.c, 1, 1});
      add(q + ".pwconv1.bias", {g.c});
    }
    const std::string q = p + "." + std::to_string(kBlocks[si] + 2);  // + 1 is to1d (no parameters)
    const int hC = g.hC;
    add(q + ".red_dim_conv.0.weight", {hC, kD, 1});
    add(q + ".red_dim_conv.0.bias", {hC});
    add(q + ".red_dim_conv.1.weight", {hC});
    add(q + ".red_dim_conv.1.bias", {hC});
    for (int j = 0; j < 4; ++j) {
      const std::string r = q + ".tcm." + std::to_string(j);
      add(r + ".dwconvs.0.weight", {hC, 1, kDwK[j]});
      add(r + ".dwconvs.0.bias", {hC});
      add_bn(r + ".norm", hC);
      add(r + ".pwconv1.weight", {hC, hC, 1});
      add(r + ".pwconv1.bias", {hC});
    }
    const std::string r = q + ".tcm.4";
    for (const char* proj : {"k_proj", "v_proj", "q_proj", "out_proj"}) {
      add(r + ".attention." + proj + ".weight", {hC, hC});
      add(r + ".attention." + proj + ".bias", {hC});
    }
    add(r + ".layer_norm.weight", {hC});
    add(r + ".layer_norm.bias", {hC});
    for (const char* l : {"intermediate_dense", "output_dense"}) {
      add(r + ".feed_forward." + l + ".weight", {hC, hC});
      add(r + ".feed_forward." + l + ".bias", {hC});
    }
    add(r + ".final_layer_norm.weight", {hC});
    add(r + ".final_layer_norm.bias", {hC});
    add(q + ".exp_dim_conv.weight", {kD, hC, 1});
    add(q + ".exp_dim_conv.bias", {kD});
  }
  add("pool.linear1.weight", {128, 3 * kD, 1});
  add("pool.linear1.bias", {128});
  add("pool.linear2.weight", {kD, 128, 1});
  add("pool.linear2.bias", {kD});
  add("seg_1.weight", {embed_dim, 2 * kD});
  add("seg_1.bias", {embed_dim});
  if (two_emb) {  // BatchNorm1d(affine=False) + seg_2
    add("seg_bn_1.running_mean", {embed_dim});
    add("seg_bn_1.running_var", {embed_dim});
    add("seg_bn_1.num_batches_tracked", {});
    add("seg_2.weight", {embed_dim, embed_dim});
    add("seg_2.bias", {embed_dim});
  }
}

// [N][K] -> [K][N]
std::vector<float> Redimnet::kmajor(const std::vector<float>& w, int N, int K) const {
  std::vector<float> t((size_t)N * K);
  for (int n = 0; n < N; ++n)
    for (int k = 0; k < K; ++k) t[(size_t)k * N + n] = w[(size_t)n * K + k];
  return t;
}

// Linear / 1x1 conv [N][K] for the shared GEMM, N padded to a multiple of 64 with zero rows (their
// output columns are zeros nothing reads)
ConvW Redimnet::lin(const std::vector<float>& w, const std::vector<float>& b, int N, int K) {
  const int Np = round_up(N, 64);
  std::vector<float> wp((size_t)Np * K, 0.f), bp(Np, 0.f);
  std::copy(w.begin(), w.begin() + (size_t)N * K, wp.begin());
  std::copy(b.begin(), b.begin() + N, bp.begin());
  return pack_conv(wp, Np, K, 1, bp.data(), "");
}

// p.dwconvs.0 [C][gin][taps] + p.norm folded -> tap-major [taps * gin][C] and its bias; p.pwconv1 k-major
Redimnet::Pw Redimnet::fold_dw(const std::string& p, int C, int gin, int taps) {
  std::vector<double> sc, sh;
  bn_affine(p + ".norm", sc, sh);
  const auto& w = P(p + ".dwconvs.0.weight");
  const auto& b = P(p + ".dwconvs.0.bias");
  std::vector<float> wd((size_t)taps * gin * C), bd(C);
  for (int co = 0; co < C; ++co) {
    for (int ci = 0; ci < gin; ++ci)
      for (int tap = 0; tap < taps; ++tap)
        wd[((size_t)tap * gin + ci) * C + co] = (float)(w[((size_t)co * gin + ci) * taps + tap] * sc[co]);
    bd[co] = (float)(b[co] * sc[co] + sh[co]);
  }
  Pw o;
  o.wd = dev.upload(wd);
  o.bd = dev.upload(bd);
  o.wp = dev.upload(kmajor(P(p + ".pwconv1.weight"), C, C));
  o.bp = dev.upload(P(p + ".pwconv1.bias"));
  return o;
}

void Redimnet::finalize() {
  for (int i = 0; i <= kStages; ++i) {  // softmax over the i + 1 inputs, per channel (f64)
    const auto& w = P("backbone.inputs_weights." + std::to_string(i));
    const int n = i + 1;
    std::vector<float> o((size_t)n * kD, 1.f);
    if (i > 0)
      for (int j = 0; j < kD; ++j) {
        double mx = w[j], sum = 0;
        for (int k = 1; k < n; ++k) mx = std::max(mx, (double)w[(size_t)k * kD + j]);
        for (int k = 0; k < n; ++k) sum += std::exp((double)w[(size_t)k * kD + j] - mx);
        for (int k = 0; k < n; ++k) o[(size_t)k * kD + j] = (float)(std::exp((double)w[(size_t)k * kD + j] - mx) / sum);
      }
    sw[i] = dev.upload(o);
  }
  stem_w = dev.upload(kmajor(P("backbone.stem.0.weight"), kC0, 9));  // [tap][16], tap = kf * 3 + kt
  stem_b = dev.upload(P("backbone.stem.0.bias"));
  stem_g = dev.upload(P("backbone.stem.1.weight"));
  stem_beta = dev.upload(P("backbone.stem.1.bias"));
  for (int si = 0; si < kStages; ++si) {
    Stage& g = st[si];
    const std::string p = "backbone.stage" + std::to_string(si);
    WSP_CHECK(rd_block2d_supported(g.F, g.c) && rd_attn_supported(g.hC / kHeads), "ReDimNet: no kernel for stage " + p);
    {  // [c][cin][s] -> k-major, k = kf * cin + ci
      const auto& w = P(p + ".0.weight");
      const int gw = g.c;
      std::vector<float> wt((size_t)gw * gw);
      for (int co = 0; co < g.c; ++co)
        for (int ci = 0; ci < g.cin; ++ci)
          for (int kf = 0; kf < g.s; ++kf) wt[(size_t)(kf * g.cin + ci) * gw + co] = w[((size_t)co * g.cin + ci) * g.s + kf];
      g.ew = dev.upload(wt);
      g.eb = dev.upload(P(p + ".0.bias"));
    }
    for (int bi = 0; bi < kBlocks[si]; ++bi) g.b2[bi] = fold_dw(p + "." + std::to_string(bi + 1) + ".conv_block", g.c, 4, 9);
    const std::string q = p + "." + std::to_string(kBlocks[si] + 2);
    const int hC = g.hC;
    g.red = lin(P(q + ".red_dim_conv.0.weight"), P(q + ".red_dim_conv.0.bias"), hC, kD);
    g.ln0_g = dev.upload(P(q + ".red_dim_conv.1.weight"));
    g.ln0_b = dev.upload(P(q + ".red_dim_conv.1.bias"));
    for (int j = 0; j < 4; ++j) g.b1[j] = fold_dw(q + ".tcm." + std::to_string(j), hC, 1, kDwK[j]);
    const std::string r = q + ".tcm.4";
    {  // one GEMM for q, k, v: columns [q | k | v]
      std::vector<float> w, b;
      for (const char* proj : {"q_proj", "k_proj", "v_proj"}) {
        const auto& pw = P(r + ".attention." + proj + ".weight");
        const auto& pb = P(r + ".attention." + proj + ".bias");
        w.insert(w.end(), pw.begin(), pw.end());
        b.insert(b.end(), pb.begin(), pb.end());
      }
      g.qkv = lin(w, b, 3 * hC, hC);
    }
    g.outp = lin(P(r + ".attention.out_proj.weight"), P(r + ".attention.out_proj.bias"), hC, hC);
    g.ln1_g = dev.upload(P(r + ".layer_norm.weight"));
    g.ln1_b = dev.upload(P(r + ".layer_norm.bias"));
    g.ff1 = lin(P(r + ".feed_forward.intermediate_dense.weight"), P(r + ".feed_forward.intermediate_dense.bias"), hC, hC);
    g.ff2 = lin(P(r + ".feed_forward.output_dense.weight"), P(r + ".feed_forward.output_dense.bias"), hC, hC);
    g.ln2_g = dev.upload(P(r + ".final_layer_norm.weight"));
    g.ln2_b = dev.upload(P(r + ".final_layer_norm.bias"));
    g.exp = lin(P(q + ".exp_dim_conv.weight"), P(q + ".exp_dim_conv.bias"), kD, hC);
  }
  // ASTP with global context, as ECAPA's: the mean / std columns of linear1 are constant over T
  // and become a per-utterance row bias (which carries linear1's bias)
  const auto& l1 = P("pool.linear1.weight");
  std::vector<float> wx((size_t)128 * kD);
  for (int n = 0; n < 128; ++n) std::copy(l1.begin() + (size_t)n * 3 * kD, l1.begin() + (size_t)n * 3 * kD + kD, wx.begin() + (size_t)n * kD);
  pool1 = pack_conv(wx, 128, kD, 1, P("pool.linear1.bias").data(), "");
  pool1_ctx = pack_lin(l1.data() + kD, 128, 2 * kD, 3 * kD, P("pool.linear1.bias").data());
  pool2 = pack_conv(P("pool.linear2.weight"), kD, 128, 1, P("pool.linear2.bias").data(), "");
  seg1 = pack_lin(P("seg_1.weight").data(), embed_dim, 2 * kD, 2 * kD, P("seg_1.bias").data());
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

Redimnet::Ws Redimnet::ws_layout(int B, int T, float* base) const {
  WsCursor c{base};
  Ws w;
  w.bc = chunk_for(B, (size_t)T * kD * sizeof(float));
  const size_t M = (size_t)w.bc * T, bc = w.bc;
  int hmax = 0, qmax = 0;
  for (const Stage& g : st) hmax = std::max(hmax, g.hCp), qmax = std::max(qmax, g.qkvp);
  for (float*& o : w.O) o = c.take(M * kD);  // every stage's 1-D output stays: later stages weight them all
  for (float*& p : w.P) p = c.take(M * kD);  // a stage's 2-D ping-pong pair; the pooling input and its logits
  for (float*& h : w.h) h = c.take(M * hmax);
  w.qkv = c.take(M * qmax);
  w.att = c.take(M * hmax);
  w.tmp = c.take(M * hmax);
  w.patt = c.take(M * 128);
  w.gstats = c.take(bc * 2 * kD);
  w.rowb = c.take(bc * 128);
  w.pooled = c.take(bc * 2 * kD);
  w.E1 = c.take(bc * embed_dim);
  w.scratch_floats = small_linear_scratch_floats((int)bc, embed_dim, 2 * kD);
  w.scratch = c.take(w.scratch_floats);
  w.floats = c.off;
  return w;
}

void Redimnet::forward(const float* feats, int B, int T, float* embed, float* ws, hipStream_t s) {
  const Ws W = ws_layout(B, T, ws);
  for (int b0 = 0; b0 < B; b0 += W.bc) {
    const int nb = std::min(W.bc, B - b0), M = nb * T;
    const double rows = M;
    run("rd_stem", 2.0 * rows * kD * 9, s, [&] {
      launch_rd_stem({feats + (size_t)b0 * T * kF0, nb, T, kF0, stem_w, stem_b, stem_g, stem_beta, (float)kLnEps, W.O[0], kD}, s);
    });
    auto weighted = [&](int n, int gw, const float* wt, const float* bias, float* out) {
      RdEntryArgs e{};
      for (int i = 0; i < n; ++i) e.in[i] = W.O[i];
      e.ld_in = kD, e.n = n, e.sw = sw[n - 1], e.rows = M, e.gw = gw, e.wt = wt, e.bias = bias, e.out = out, e.ldo = kD;
      run(gw ? "rd_entry" : "rd_wsum", 2.0 * rows * kD * (n + gw), s, [&] { launch_rd_entry(e, s); });
    };
    for (int si = 0; si < kStages; ++si) {
      const Stage& g = st[si];
      float *x = W.P[0], *o = W.P[1];
      weighted(si + 1, g.c, g.ew, g.eb, x);
      for (const Pw& b : g.b2) {
        const RdBlock2dArgs a{x, kD, nb, T, g.F, g.c, b.wd, b.bd, b.wp, b.bp, o, kD};
        run("rd_block2d", 2.0 * rows * kD * (36 + g.c), s, [&] { launch_rd_block2d(a, s); });
        std::swap(x, o);
      }
      const int hC = g.hC, ld = g.hCp;
      float *h = W.h[0], *h2 = W.h[1];
      auto ln = [&](const float* in, const float* add, const float* gamma, const float* beta, float* out) {
        const RdLnArgs a{in, ld, add, ld, gamma, beta, (float)kLnEps, out, ld, M, hC};
        run("rd_ln", 0, s, [&] { launch_rd_layernorm(a, s); });
      };
      gemm("rd_red", g.red, x, kD, h2, ld, M, T, 1, 0, kActNone, s, nullptr, 0);
      ln(h2, nullptr, g.ln0_g, g.ln0_b, h);
      for (int j = 0; j < 4; ++j) {
        const RdBlock1dArgs a{h, ld, nb, T, hC, kDwK[j], g.b1[j].wd, g.b1[j].bd, g.b1[j].wp, g.b1[j].bp, h2, ld};
        run("rd_block1d", 2.0 * rows * hC * (kDwK[j] + hC), s, [&] { launch_rd_block1d(a, s); });
        std::swap(h, h2);
      }
      // post-LN transformer layer: h = LN(h + attn(h)); h = LN(h + FFN(h))
      gemm("rd_qkv", g.qkv, h, ld, W.qkv, g.qkvp, M, T, 1, 0, kActNone, s, nullptr, 0);
      const int dh = hC / kHeads;
      const RdAttnArgs at{W.qkv, g.qkvp, nb, T, kHeads, dh, 1.f / std::sqrt((float)dh), W.att, ld};
      run("rd_attn", 4.0 * rows * T * hC, s, [&] { launch_rd_attn(at, s); });
      gemm("rd_lin", g.outp, W.att, ld, W.tmp, ld, M, T, 1, 0, kActNone, s, nullptr, 0);
      ln(h, W.tmp, g.ln1_g, g.ln1_b, h2);
      gemm("rd_lin", g.ff1, h2, ld, W.tmp, ld, M, T, 1, 0, kActNone, s, nullptr, 0);
      run("rd_gelu", 0, s, [&] { launch_rd_gelu_tanh(W.tmp, ld, M, hC, s); });
      gemm("rd_lin", g.ff2, W.tmp, ld, W.att, ld, M, T, 1, 0, kActNone, s, nullptr, 0);
      ln(h2, W.att, g.ln2_g, g.ln2_b, h);
      {  // expansion + skip (the stage's 2-D output), written as the stage's 1-D output
        ConvGemmArgs e{};
        one_operand(e, h, ld, g.exp.cin);
        fill(e, g.exp, M, T, 1, 0, W.O[si + 1], kD, kActNone, nullptr, true, nullptr, 0);
        e.res = x;
        e.ldres = kD;
        run("rd_exp", 2.0 * rows * kD * hC, s, [&] { launch(e, g.exp, s); });
      }
    }
    // the backbone's output, then ASTP with global context and the embedding layers
    float *xp = W.P[0], *logit = W.P[1];
    weighted(kStages + 1, 0, nullptr, nullptr, xp);
    run("glob_ctx", 0, s, [&] {
      launch_frame_stats(xp, kD, nb, T, kD, W.gstats, 2 * kD, 1, kD, s);
      launch_small_linear({W.gstats, 2 * kD, pool1_ctx.wt, pool1_ctx.bias, W.rowb, 128, nb, 2 * kD, 128, 0}, s);
    });
    gemm("pool_linear1", pool1, xp, kD, W.patt, 128, M, T, 1, 0, kActTanh, s, nullptr, 0, W.rowb, false);
    gemm("pool_linear2", pool2, W.patt, 128, logit, kD, M, T, 1, 0, kActNone, s, nullptr, 0);
    run("astp", 0, s, [&] { launch_astp_pool(logit, xp, nb, T, kD, W.pooled, s); });
    run("head", 0, s, [&] {
      float* e_out = embed + (size_t)b0 * embed_dim;
      launch_small_linear({W.pooled, 2 * kD, seg1.wt, seg1.bias, two_emb ? W.E1 : e_out, embed_dim, nb, 2 * kD, embed_dim,
                           two_emb ? 1 : 0, W.scratch_floats ? W.scratch : nullptr, W.scratch_floats},
                          s);
      if (two_emb)
        launch_small_linear({W.E1, embed_dim, seg2.wt, seg2.bias, e_out, embed_dim, nb, embed_dim, embed_dim, 0}, s);
    });
  }
}

}  // namespace wsp
