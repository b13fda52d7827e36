// ECAPA-TDNN: parameter table, weight folding / packing, workspace and forward schedule.
//
// Forward = wespeaker/models/ecapa_tdnn.py:208-234, channels-last:
//   layer1  Conv1dReluBn(F->C, k5)                        -> x1   [M][C]
//   layerL  SE_Res2Block(dil L):  c1 (1x1) -> h1
//           Res2 chain i=0..6: conv_k3(h1_i (+ h2_{i-1})) -> h2_i  (7 GEMMs)
//           c3 (1x1) over cat(h2_0..6, h1_7)             -> h3   (no copy)
//           SE: frame mean -> FC relu -> FC sigmoid -> x_{L} + h3 * g
//           (the last block: g4 * h3 alone, or with gate_fold nothing — conv reads h3 and g4;
//           the first two with seam_fold: the next block's c1 forms the sum as it stages its A
//           operand and writes it on the way — no pass of its own)
//   conv    1x1 over cat(x2, x3, x4) (no copy), ReLU      -> xp   [M][1536]
//   ASTP    [GLOB: frame mean/std -> per-utterance bias]  -> tanh(W1 xp) -> W2
//           -> online-softmax attentive mean/std          -> [B][3072]
//   head    BN(3072) + Linear (+ bn2) folded into one GEMV -> embed [B][D]
// XI_VEC_ECAPA_TDNN_*: the same trunk; the pooling stage is XI (pooling_layers.py class XI):
//   XI      lin1 (1536 -> 256, ReLU -> BN) -> lin2 (256 -> 1536) -> launch_xi_pool -> [B][1536]
//   head    BN(1536) + Linear (+ bn2), the same fold with K = 1536
#include "astp_fused.h"
#include "model_impl.h"
#include "res2_chain.h"
#include "xi_pool.h"

namespace wsp {

namespace {
struct Ecapa final : Model::Impl {
  using Impl::Impl;
  int C = 512;
  bool glob = false;
  bool xi = false;  // XI pooling instead of ASTP (the XI_VEC_ECAPA_TDNN_* names)
  ConvW layer1;
  struct Block {
    ConvW c1, c3, res2[7];
    LinW se1, se2;
    // the 7 Res2Net convs packed for res2_chain.hip (one launch per block)
    void* r2w = nullptr;
    float *r2b = nullptr, *r2s = nullptr, *r2t = nullptr;
  } blk[3];
  ConvW conv, pool1, pool2;
  ConvW conv_g;                // conv with W_b + W_c in its middle third (option "cat_gate")
  void* pool2_frag = nullptr;  // pool.linear2 in MFMA B-fragment order for astp_fused.hip
  LinW pool1_ctx;
  float *prior_mean = nullptr, *prior_logprec = nullptr;  // XI (pool1 / pool2 hold lin1 / lin2)
  LinW head;
  int pooled_dim() const { return xi ? 1536 : 3072; }

  void build_params() override;
  void pack_res2(Block& b, const std::string& p, int w);
  void finalize() override;
  int chunk(int B, int T) const;
  size_t ws_floats(int B, int T) const override;
  void forward(const float* feats, int B, int T, float* embed, float* ws, hipStream_t s) override;
  // seg (device [B+1] row offsets) non-null: ragged batch of M rows; T unused by the
  // kernels then (per-utterance lengths come from seg).
  void forward_chunk(const float* feats, int B, int T, float* embed, float* ws, hipStream_t s,
                     const int* seg = nullptr, int M_seg = 0);
  int min_frames() const override { return xi ? 1 : 2; }
  bool has_segments() const override { return true; }
  size_t ws_floats_segments(int B, int M) const override;
  void forward_segments(const float* feats, int B, const int* seg, int M, float* embed, float* ws,
                        hipStream_t s) override {
    forward_chunk(feats, B, 1, embed, ws, s, seg, M);  // T unused when segmented
  }
};
}  // namespace

Model::Impl* make_ecapa(const std::string& arch, int feat_dim, int embed_dim, bool emb_bn, bool two_emb) {
  const bool xi = arch == "XI_VEC_ECAPA_TDNN_c512" || arch == "XI_VEC_ECAPA_TDNN_c1024";
  if (!xi && arch != "ECAPA_TDNN_c512" && arch != "ECAPA_TDNN_GLOB_c512" && arch != "ECAPA_TDNN_c1024" &&
      arch != "ECAPA_TDNN_GLOB_c1024")
    return nullptr;
  WSP_CHECK(!(xi && two_emb), "XI_VEC_ECAPA_TDNN has no two_emb_layer");
  WSP_CHECK(feat_dim > 0 && feat_dim % 4 == 0, "ECAPA feat_dim must be a positive multiple of 4");
  WSP_CHECK(embed_dim > 0, "embed_dim must be positive");
  Ecapa* m = new Ecapa(arch, feat_dim, embed_dim, emb_bn, two_emb);
  m->opt.x3_variant = 7;  // 6 (the 256 x 256 tile on 16x16x32 MFMAs, r3) with LDS-DMA staging (r4)
  m->C = (arch.find("c1024") != std::string::npos) ? 1024 : 512;
  m->glob = arch.find("GLOB") != std::string::npos;
  m->xi = xi;
  return m;
}

void Ecapa::build_params() {
  const int64_t C = this->C, w = C / 8;
  add("layer1.conv.weight", {C, feat_dim, 5});
  add("layer1.conv.bias", {C});
  add_bn("layer1.bn", C);
  for (int li = 2; li <= 4; ++li) {
    const std::string p = "layer" + std::to_string(li) + ".se_res2block";
    add(p + ".0.conv.weight", {C, C, 1});
    add(p + ".0.conv.bias", {C});
    add_bn(p + ".0.bn", C);
    for (int i = 0; i < 7; ++i) {
      add(p + ".1.convs." + std::to_string(i) + ".weight", {w, w, 3});
      add(p + ".1.convs." + std::to_string(i) + ".bias", {w});
    }
    for (int i = 0; i < 7; ++i) add_bn(p + ".1.bns." + std::to_string(i), w);
    add(p + ".2.conv.weight", {C, C, 1});
    add(p + ".2.conv.bias", {C});
    add_bn(p + ".2.bn", C);
    add(p + ".3.linear1.weight", {128, C});
    add(p + ".3.linear1.bias", {128});
    add(p + ".3.linear2.weight", {C, 128});
    add(p + ".3.linear2.bias", {C});
  }
  add("conv.weight", {1536, 3 * C, 1});
  add("conv.bias", {1536});
  if (xi) {
    add("pool.prior_mean", {1, 1536});
    add("pool.prior_logprec", {1, 1536});
    add("pool.lin1_relu_bn.0.weight", {256, 1536, 1});
    add("pool.lin1_relu_bn.0.bias", {256});
    add_bn("pool.lin1_relu_bn.2", 256);
    add("pool.lin2.weight", {1536, 256, 1});
    add("pool.lin2.bias", {1536});
  } else {
    add("pool.linear1.weight", {128, glob ? 4608 : 1536, 1});
    add("pool.linear1.bias", {128});
    add("pool.linear2.weight", {1536, 128, 1});
    add("pool.linear2.bias", {1536});
  }
  add_bn("bn", pooled_dim());
  add("linear.weight", {embed_dim, pooled_dim()});
  add("linear.bias", {embed_dim});
  if (emb_bn) add_bn("bn2", embed_dim);
}

// Res2Net chain weights for res2_chain.hip (pack::frag_res2); conv bias and eval-BN affine per
// step [7][w].
void Ecapa::pack_res2(Block& b, const std::string& p, int w) {
  const std::vector<float>* W[7];
  std::vector<float> bias((size_t)7 * w), sc((size_t)7 * w), sh((size_t)7 * w);
  for (int i = 0; i < 7; ++i) {
    const std::string ci = p + ".1.convs." + std::to_string(i);
    W[i] = &P(ci + ".weight");
    const auto& bb = P(ci + ".bias");
    std::vector<double> s, t;
    bn_affine(p + ".1.bns." + std::to_string(i), s, t);
    for (int n = 0; n < w; ++n) {
      bias[(size_t)i * w + n] = bb[n];
      sc[(size_t)i * w + n] = (float)s[n];
      sh[(size_t)i * w + n] = (float)t[n];
    }
  }
  b.r2w = dev.upload_u16(pack::frag_res2(W, w));
  b.r2b = dev.upload(bias);
  b.r2s = dev.upload(sc);
  b.r2t = dev.upload(sh);
}

void Ecapa::finalize() {
  const int w = C / 8;
  layer1 = pack_conv(P("layer1.conv.weight"), C, feat_dim, 5, P("layer1.conv.bias").data(), "layer1.bn");
  for (int li = 0; li < 3; ++li) {
    const std::string p = "layer" + std::to_string(li + 2) + ".se_res2block";
    Block& b = blk[li];
    b.c1 = pack_conv(P(p + ".0.conv.weight"), C, C, 1, P(p + ".0.conv.bias").data(), p + ".0.bn");
    for (int i = 0; i < 7; ++i) {
      const std::string ci = p + ".1.convs." + std::to_string(i);
      b.res2[i] = pack_conv(P(ci + ".weight"), w, w, 3, P(ci + ".bias").data(), p + ".1.bns." + std::to_string(i));
    }
    if (res2_chain_supported(w, li + 2)) pack_res2(b, p, w);
    b.c3 = pack_conv(P(p + ".2.conv.weight"), C, C, 1, P(p + ".2.conv.bias").data(), p + ".2.bn");
    b.se1 = pack_lin(P(p + ".3.linear1.weight").data(), 128, C, C, P(p + ".3.linear1.bias").data());
    b.se2 = pack_lin(P(p + ".3.linear2.weight").data(), C, 128, 128, P(p + ".3.linear2.bias").data());
  }
  conv = pack_conv(P("conv.weight"), 1536, 3 * C, 1, P("conv.bias").data(), "");
  {
    std::vector<float> wg = P("conv.weight");  // [1536][3C]
    for (int n = 0; n < 1536; ++n)
      for (int c = 0; c < C; ++c) {
        float* r = wg.data() + (size_t)n * 3 * C;
        r[C + c] = (float)((double)r[C + c] + (double)r[2 * C + c]);
      }
    conv_g = pack_conv(wg, 1536, 3 * C, 1, P("conv.bias").data(), "");
  }
  if (xi) {
    pool1 = pack_conv(P("pool.lin1_relu_bn.0.weight"), 256, 1536, 1, P("pool.lin1_relu_bn.0.bias").data(),
                      "pool.lin1_relu_bn.2");
    pool2 = pack_conv(P("pool.lin2.weight"), 1536, 256, 1, P("pool.lin2.bias").data(), "");
    prior_mean = dev.upload(P("pool.prior_mean"));
    prior_logprec = dev.upload(P("pool.prior_logprec"));
  } else {
    const auto& l1 = P("pool.linear1.weight");
    const int l1k = glob ? 4608 : 1536;
    std::vector<float> wx((size_t)128 * 1536);
    for (int n = 0; n < 128; ++n)
      for (int k = 0; k < 1536; ++k) wx[(size_t)n * 1536 + k] = l1[(size_t)n * l1k + k];
    pool1 = pack_conv(wx, 128, 1536, 1, P("pool.linear1.bias").data(), "");
    if (glob) {
      // columns 1536..4607 multiply the (constant over T) mean/std context:
      // folded into a per-utterance bias computed by small_linear.
      pool1_ctx = pack_lin(l1.data() + 1536, 128, 3072, l1k, P("pool.linear1.bias").data());
    }
    pool2 = pack_conv(P("pool.linear2.weight"), 1536, 128, 1, P("pool.linear2.bias").data(), "");
    pool2_frag = pack_frag(P("pool.linear2.weight"), 1536, 128);
  }
  // head: y = Linear(BN(p)) [-> bn2] folded to y = W' p + b'
  {
    std::vector<double> s, t;
    bn_affine("bn", s, t);
    const auto& W = P("linear.weight");
    const auto& bb = P("linear.bias");
    const int D = embed_dim;
    std::vector<double> s2(D, 1.0), t2(D, 0.0);
    if (emb_bn) bn_affine("bn2", s2, t2);
    const int K = pooled_dim();
    std::vector<float> wf((size_t)D * K), bf(D);
    for (int n = 0; n < D; ++n) {
      double acc = bb[n];
      for (int k = 0; k < K; ++k) {
        const double wv = W[(size_t)n * K + k];
        wf[(size_t)n * K + k] = (float)(s2[n] * wv * s[k]);
        acc += wv * t[k];
      }
      bf[n] = (float)(s2[n] * acc + t2[n]);
    }
    head = pack_lin(wf.data(), D, K, K, bf.data());
  }
}

// utterances per ECAPA forward chunk (uniform batches): the widest activation operand is the
// [M][1536] ASTP input / logits; larger batches run as consecutive chunks over one chunk-sized
// workspace, as the other families
int Ecapa::chunk(int B, int T) const {
  return chunk_for(B, (size_t)T * std::max(C, 1536) * sizeof(float));
}

namespace {
// M = frame rows of the batch (B * T, or the segment total)
struct EcapaWs {
  float *x[5], *h1, *h2, *h3, *gmean, *ghid, *gate, *xp, *att, *logit, *gstats, *rowb, *pooled;
  double* sesum;  // SE column-sum partials (f64)
  size_t floats;
};
// xi: the attention hidden layer is 256 wide (XI's lin1) instead of 128
EcapaWs ecapa_ws(size_t C, size_t B, size_t M, float* base, bool xi) {
  WsCursor c{base};
  EcapaWs w;
  w.x[0] = nullptr;
  for (int i = 1; i <= 4; ++i) w.x[i] = c.take(M * C);
  w.h1 = c.take(M * C);
  w.h2 = c.take(M * C);
  w.h3 = c.take(M * C);
  w.gmean = c.take(B * C);
  w.ghid = c.take(B * 128);
  w.gate = c.take(B * C);
  w.xp = c.take(M * 1536);
  w.att = c.take(M * (xi ? 256 : 128));
  w.logit = c.take(M * 1536);
  w.gstats = c.take(B * 3072);
  w.rowb = c.take(B * 128);
  w.pooled = c.take(B * 3072);
  w.sesum = reinterpret_cast<double*>(c.take(((M + 127) / 128) * 2 * C * 2));
  w.floats = c.off;
  return w;
}
}  // namespace

size_t Ecapa::ws_floats(int B, int T) const {
  const size_t bc = chunk(B, T);
  return ecapa_ws(C, bc, bc * T, nullptr, xi).floats;
}

size_t Ecapa::ws_floats_segments(int B, int M) const { return ecapa_ws(C, B, M, nullptr, xi).floats; }

void Ecapa::forward(const float* feats, int B, int T, float* embed, float* ws, hipStream_t s) {
  const int bc = chunk(B, T);
  for (int c0 = 0; c0 < B; c0 += bc)
    forward_chunk(feats + (size_t)c0 * T * feat_dim, std::min(bc, B - c0), T, embed + (size_t)c0 * embed_dim, ws, s);
}

void Ecapa::forward_chunk(const float* feats, int B, int T, float* embed, float* ws, hipStream_t s,
                          const int* seg, int M_seg) {
  const int M = seg ? M_seg : B * T, w = C / 8;
  const EcapaWs W = ecapa_ws(C, B, M, ws, xi);
  float* const* x = W.x;
  float *h1 = W.h1, *h2 = W.h2, *h3 = W.h3, *xp = W.xp;
  // SE squeeze fused into conv3's epilogue (per-utterance f64 column sums) on the
  // bf16x3 path for uniform batches whose utterances span >= one block of rows
  const int se_bm = opt.precision == 1 ? conv_gemm_x3_block_rows(ConvGemmArgs{.N = C}, opt.x3_variant) : 0;
  const bool se_fused = opt.precision == 1 && !seg && T >= se_bm;
  // a GEMM whose three A slots (set by the caller) cat / add different [M][C] tensors
  auto gemm3 = [&](const char* tag, ConvGemmArgs& g, const ConvW& cw, int dil, int pad, float* out, int ldo) {
    g.lda[0] = g.lda[1] = g.lda[2] = C;
    fill(g, cw, M, T, dil, pad, out, ldo, kActRelu, nullptr, true, seg, B);
    run(tag, 2.0 * M * cw.N * cw.K, s, [&] { launch(g, cw, s); });
  };

  // conv_cat's operands; with gate_fold its third slot is h3 of the last block with the SE gate
  // attached (multiplied in as the A fragments are read), where the GEMM kernel takes a gate
  ConvGemmArgs gcat{};
  gcat.amode = kACat;
  gcat.a[0] = x[2];
  gcat.a[1] = x[3];
  gcat.a[2] = x[4];
  gcat.cseg[1] = C;
  gcat.cseg[2] = 2 * C;
  gcat.cseg[3] = 3 * C;
  gcat.lda[0] = gcat.lda[1] = gcat.lda[2] = C;
  const ConvW& wcat = opt.cat_gate ? conv_g : conv;
  bool fold = false;
  if (opt.cat_gate && opt.gate_fold && opt.precision == 1) {
    ConvGemmArgs g = gcat;
    g.a[2] = h3;
    g.gate = W.gate;
    g.ldg = C;
    g.gate_k0 = 2 * C;
    fill(g, wcat, M, T, 1, 0, xp, 1536, kActRelu, nullptr, true, seg, B);
    fold = conv_gemm_x3_gate_ok(g, opt.x3_variant);
    if (fold) gcat = g;
  }

  gemm("layer1", layer1, feats, feat_dim, x[1], C, M, T, 1, 2, kActRelu, s, seg, B);
  // seam_fold: the previous block left its output unwritten — gseam is this block's c1 with
  // A = x + g (.) h3 (ConvGemmArgs::seam_h), which also stores that sum to this block's xin
  ConvGemmArgs gseam{};
  bool seam = false;
  for (int li = 0; li < 3; ++li) {
    const Block& b = blk[li];
    const int dil = li + 2;
    const float* xin = x[li + 1];
    if (seam) {
      // one launch, both jobs: the block output it materialises (se.scale) and the C x C GEMM
      run("se.scale", 0, s, [&] {
        run("seam", 0, s, [&] { run("conv1x1_CxC", 2.0 * M * C * C, s, [&] { launch(gseam, b.c1, s); }); });
      });
      seam = false;
    } else {
      gemm("conv1x1_CxC", b.c1, xin, C, h1, C, M, T, 1, 0, kActRelu, s, seg, B, nullptr, true, 1);
    }
    if (opt.precision == 1 && opt.res2_fused && b.r2w) {
      // the whole chain in one launch (res2_chain.hip)
      Res2Args r{};
      r.x = h1;
      r.out = h2;
      r.ldx = r.ldo = C;
      r.M = M;
      r.T = T;
      r.dil = dil;
      r.variant = w == 128 ? opt.res2_variant : std::min(opt.res2_variant, 3);
      r.rout = res2_chain_rout(dil, r.variant, M);
      r.seg = seg;
      r.nseg = B;
      r.w = b.r2w;
      r.bias = b.r2b;
      r.scale = b.r2s;
      r.shift = b.r2t;
      run("res2_k3", 7 * 2.0 * M * w * 3 * w, s, [&] { launch_res2_chain(r, w, s); });
    } else {
      for (int i = 0; i < 7; ++i) {  // h1_0 alone, then h1_i + h2_{i-1}
        ConvGemmArgs g{};
        g.amode = i == 0 ? kACat : kAAdd;
        if (i == 0) {
          one_operand(g, h1, C, w);
        } else {
          g.a[0] = h1 + i * w;
          g.a[1] = h2 + (i - 1) * w;
          g.a[2] = h1;
        }
        gemm3("res2_k3", g, b.res2[i], dil, dil, h2 + i * w, C);
      }
    }
    {
      ConvGemmArgs g{};
      g.amode = kACat;
      g.a[0] = h2;
      g.a[1] = h1 + 7 * w;
      g.a[2] = h1;
      g.cseg[1] = 7 * w;
      g.cseg[2] = g.cseg[3] = C;
      g.role = 1;
      if (se_fused) g.colsum = W.sesum;
      gemm3("conv1x1_CxC", g, b.c3, 1, 0, h3, C);
    }
    run("se", 0, s, [&] {
      if (se_fused) launch_colsum_mean(W.sesum, se_bm, T, B, C, W.gmean, C, s);
      else launch_frame_stats(h3, C, B, T, C, W.gmean, C, 0, 0, s, seg);
      launch_small_linear({W.gmean, C, b.se1.wt, b.se1.bias, W.ghid, 128, B, C, 128, 1}, s);
      launch_small_linear({W.ghid, 128, b.se2.wt, b.se2.bias, W.gate, C, B, 128, C, 3}, s);
    });
    // cat_gate: the last block stores only g4 * h3 (conv_cat adds out3 through its weights);
    // gate_fold: not even that — conv_cat reads h3 and the gate (x[4] stays unwritten)
    if (li == 2 && fold) continue;
    if (li < 2 && opt.seam_fold && opt.precision == 1) {
      ConvGemmArgs g{};
      one_operand(g, xin, C, C);
      g.role = 1;
      g.seam_h = h3;
      g.ld_seam_h = C;
      g.gate = W.gate;
      g.ldg = C;
      g.seam_out = x[li + 2];
      g.ld_seam_out = C;
      fill(g, blk[li + 1].c1, M, T, 1, 0, h1, C, kActRelu, nullptr, true, seg, B);
      seam = conv_gemm_x3_seam_ok(g, opt.x3_variant);
      if (seam) {
        gseam = g;
        continue;
      }
    }
    run("se.scale", 0, s, [&] {
      launch_residual_scale(opt.cat_gate && li == 2 ? nullptr : xin, h3, W.gate, x[li + 2], B, T, C, s, seg, M);
    });
  }
  gemm3("conv_cat", gcat, wcat, 1, 0, xp, 1536);
  if (glob) {
    run("glob_ctx", 0, s, [&] {
      launch_frame_stats(xp, 1536, B, T, 1536, W.gstats, 3072, 1, 1536, s, seg);
      launch_small_linear({W.gstats, 3072, pool1_ctx.wt, pool1_ctx.bias, W.rowb, 128, B, 3072, 128, 0}, s);
    });
  }
  if (xi) {
    // XI: logits z = lin2(BN(ReLU(lin1 xp))), then the Gaussian posterior mean over frames + prior
    gemm("xi_lin1", pool1, xp, 1536, W.att, 256, M, T, 1, 0, kActRelu, s, seg, B);
    gemm("xi_lin2", pool2, W.att, 256, W.logit, 1536, M, T, 1, 0, kActNone, s, seg, B);
    const XiPoolArgs a{W.logit, 1536, xp, 1536, prior_mean, prior_logprec, B, T, 1536, seg, W.pooled, 1536};
    run("xi_pool", 0, s, [&] { launch_xi_pool(a, s); });
    run("head", 0, s, [&] {
      launch_small_linear({W.pooled, 1536, head.wt, head.bias, embed, embed_dim, B, 1536, embed_dim, 0}, s);
    });
    return;
  }
  // GLOB: the context's per-utterance row bias carries pool.linear1's bias
  gemm("pool_linear1", pool1, xp, 1536, W.att, 128, M, T, 1, 0, kActTanh, s, seg, B, glob ? W.rowb : nullptr, !glob);
  if (opt.precision == 1 && opt.astp_fused) {
    // linear2 + softmax over frames + attentive mean / std in one pass (astp_fused.hip)
    AstpArgs a{W.att, xp, 1536, B, T, 1536, seg, pool2_frag, pool2.bias, 1e-7f, W.pooled};
    run("astp", 2.0 * M * 1536 * 128, s, [&] { launch_astp_fused(a, s); });
  } else {
    gemm("pool_linear2", pool2, W.att, 128, W.logit, 1536, M, T, 1, 0, kActNone, s, seg, B);
    run("astp", 0, s, [&] { launch_astp_pool(W.logit, xp, B, T, 1536, W.pooled, s, seg); });
  }
  run("head", 0, s, [&] {
    launch_small_linear({W.pooled, 3072, head.wt, head.bias, embed, embed_dim, B, 3072, embed_dim, 0}, s);
  });
}

}  // namespace wsp
