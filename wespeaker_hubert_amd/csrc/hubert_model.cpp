// HuBERT-base SSL front end runtime (arch "HuBERT_base"), and WavLM Base / Base+
// (arch "WavLM_base": the same network with a gated relative-position bias in
// every attention, attn.hip; s3prl `wavlm_base` / `wavlm_base_plus`).
//
// Replaces S3prlFrontend.forward (wespeaker/frontend/s3prl.py:80-93) with the
// s3prl `hubert` upstream (third party, restated in oracle/hubert_ref.py):
//   conv0 + GroupNorm + GELU           launch_hubert_conv0          [B][T0][512]
//   6 x strided conv + GELU            implicit GEMM (stride 2)     [B][T][512]
//   LayerNorm(512) -> Linear(512->768) layernorm + GEMM             x [B][T][768]
//   x + GELU(pos_conv(x)) -> LN        grouped GEMM (16 x 48 ch, k128) + layernorm
//   12 x post-LN transformer layer     GEMM qkv | mha | GEMM out(+x) | LN |
//                                      GEMM fc1 GELU | GEMM fc2(+x) | LN
//   Featurizer + length match          accumulated inside each hidden-state LN
// Parameters arrive under the reference checkpoint's names
// ("frontend.upstream.upstream.model." + fairseq names, "frontend.featurizer.weights").
#include <cstring>

#include "attn.h"
#include "model_impl.h"

namespace wsp {

namespace {

constexpr int kConvDim = 512, kHidden = 768, kLayers = 12, kHeads = 12, kFfn = 3072;
constexpr int kPosK = 128, kPosGroups = 16, kPosGin = kHidden / kPosGroups, kPosGout = 64;
constexpr int kConvK[7] = {10, 3, 3, 3, 3, 2, 2};
constexpr int kConvS[7] = {5, 2, 2, 2, 2, 2, 2};
constexpr int kDownsample = 320;
constexpr int kMinSamples = 800;  // s3prl MIN_SECOND (0.05 s) * 16 kHz
constexpr int kRelBuckets = 320, kRelMaxDist = 800;  // WavLM relative_attention_bias
const char* const kPre = "frontend.upstream.upstream.model.";

std::string hp(const std::string& n) { return std::string(kPre) + n; }

// Batch plan: utterance ranges of the feature extractor, their row counts per conv level, and the
// int32 offset tables.
struct HubertChunk {
  int b0 = 0, b1 = 0;
  size_t off = 0;       // index of this chunk's tables in HubertPlan::offs
  size_t rows[7] = {};  // conv-level frame rows of the chunk
  size_t samples = 0, sample0 = 0, row6 = 0;
  size_t row3 = 0;  // the chunk's first row in the batch-wide level-3 rows (cnn_tail_batch)
  int maxT0 = 0;
};
struct HubertPlan {
  int B = 0;
  size_t M = 0, Mout = 0, maxA = 0, maxB = 0;
  // batch-wide rows of conv levels 3..5 and whether CNN layers 4..6 run once over the batch
  // (their global offsets follow seg6 | fseg in offs as seg3 | seg4 | seg5)
  size_t M3 = 0, M4 = 0, M5 = 0;
  bool tail_batch = false;
  int maxChunk = 0, maxT6 = 0;
  size_t maxStats = 0;  // doubles of conv0 partial moments (hubert_conv0_stats_doubles) of the largest chunk
  std::vector<HubertChunk> chunks;
  std::vector<int> offs;
};

// channels-last [B][T][C]
struct Hubert final : Model::Impl {
  using Impl::Impl;
  // WavLM Base / Base+ (arch "WavLM_base"): HuBERT-base plus the gated relative-position bias
  bool wavlm = false;
  float* h_conv0_w = nullptr;  // [512][10]
  float *h_gn_g = nullptr, *h_gn_b = nullptr;
  ConvW h_conv[7];  // 1..6: strided feature-extractor convs (GELU epilogue)
  float *h_ln0_g = nullptr, *h_ln0_b = nullptr;
  ConvW h_proj, h_pos;
  float *h_enc_g = nullptr, *h_enc_b = nullptr;
  struct HLayer {
    ConvW qkv, out, fc1, fc2;
    float *ln1_g = nullptr, *ln1_b = nullptr, *ln2_g = nullptr, *ln2_b = nullptr;
    // LayerNorm fold (option ln_fold): fc1 on the un-normalised rows with gamma1 folded into W
    // and W beta1 into the bias; fc1_cs[n] = sum_c W'[n][c] (of the bf16 hi + lo images)
    ConvW fc1f;
    float* fc1_cs = nullptr;
    float* gate_w = nullptr;  // WavLM: [wa (64) | wb (64) | ba | bb | grep_a (12)] (attn.h launch_attn_gate)
  };
  float* h_rel_tab = nullptr;  // WavLM: [12][kAttnRelStride] bias per head over d = key - query in [-778, 778]
  std::vector<HLayer> h_layers;
  std::vector<float> h_fw;  // featurizer weight per hidden state

  void build_params() override;
  void finalize() override;
  bool owns_option(const std::string& key) const override { return key == "layer"; }
  bool is_frontend() const override { return true; }
  // wav -> frames only: Model refuses its feats -> embedding calls on a front-end handle before these
  size_t ws_floats(int, int) const override { throw InvalidArg{"front-end handle: no embedding forward"}; }
  void forward(const float*, int, int, float*, float*, hipStream_t) override { ws_floats(0, 0); }
  HubertPlan plan(int B, const int* lens) const;
  size_t ws_bytes(const HubertPlan& pl) const;  // one range's workspace slice, 256-byte granules
  void forward(const float* wav, const HubertPlan& pl, float* feats, int cmn, float* ws, hipStream_t s);
};

// the front-end entry points' way to their handle; `what`: the refusal of any other handle
Hubert& as_hubert(Model::Impl* m, const char* what) {
  Hubert* h = dynamic_cast<Hubert*>(m);
  WSP_CHECK(h, what);
  return *h;
}

}  // namespace

Model::Impl* make_hubert(const std::string& arch, int, int embed_dim, bool emb_bn, bool two_emb) {
  // s3prl HuBERT-base / WavLM Base(+) upstream + Featurizer (frontend/s3prl.py); input is
  // the waveform, output 768-dim frames (S3prlFrontend.output_size()).  WavLM_base is the
  // HuBERT-base network with a gated relative-position bias in every attention.
  if (arch != "HuBERT_base" && arch != "WavLM_base") return nullptr;
  WSP_CHECK(embed_dim == 768, arch + " output size is 768");
  Hubert* m = new Hubert(arch, 1, embed_dim, emb_bn, two_emb);
  m->wavlm = arch == "WavLM_base";
  m->opt.x3_variant = 7;  // every GEMM whose operands family 7 takes (r4), the rest on 6
  m->opt.streams = 2;     // HuBERT + ECAPA C4 chain +2.6 %
  return m;
}

void Hubert::build_params() {
  for (int i = 0; i < 7; ++i) {
    add(hp("feature_extractor.conv_layers." + std::to_string(i) + ".0.weight"),
        {kConvDim, i == 0 ? 1 : kConvDim, kConvK[i]});
    if (i == 0) {
      add(hp("feature_extractor.conv_layers.0.2.weight"), {kConvDim});
      add(hp("feature_extractor.conv_layers.0.2.bias"), {kConvDim});
    }
  }
  add(hp("layer_norm.weight"), {kConvDim});
  add(hp("layer_norm.bias"), {kConvDim});
  add(hp("post_extract_proj.weight"), {kHidden, kConvDim});
  add(hp("post_extract_proj.bias"), {kHidden});
  add(hp("encoder.pos_conv.0.bias"), {kHidden});
  add(hp("encoder.pos_conv.0.weight_g"), {1, 1, kPosK});
  add(hp("encoder.pos_conv.0.weight_v"), {kHidden, kPosGin, kPosK});
  add(hp("encoder.layer_norm.weight"), {kHidden});
  add(hp("encoder.layer_norm.bias"), {kHidden});
  for (int l = 0; l < kLayers; ++l) {
    const std::string p = "encoder.layers." + std::to_string(l) + ".";
    for (const char* proj : {"k_proj", "v_proj", "q_proj", "out_proj"}) {
      add(hp(p + "self_attn." + proj + ".weight"), {kHidden, kHidden});
      add(hp(p + "self_attn." + proj + ".bias"), {kHidden});
    }
    add(hp(p + "self_attn_layer_norm.weight"), {kHidden});
    add(hp(p + "self_attn_layer_norm.bias"), {kHidden});
    add(hp(p + "fc1.weight"), {kFfn, kHidden});
    add(hp(p + "fc1.bias"), {kFfn});
    add(hp(p + "fc2.weight"), {kHidden, kFfn});
    add(hp(p + "fc2.bias"), {kHidden});
    add(hp(p + "final_layer_norm.weight"), {kHidden});
    add(hp(p + "final_layer_norm.bias"), {kHidden});
    if (wavlm) {
      // gated relative-position bias: the bucket embedding lives in layer 0 and serves every layer
      if (l == 0) add(hp(p + "self_attn.relative_attention_bias.weight"), {kRelBuckets, kHeads});
      add(hp(p + "self_attn.grep_linear.weight"), {8, kHidden / kHeads});
      add(hp(p + "self_attn.grep_linear.bias"), {8});
      add(hp(p + "self_attn.grep_a"), {1, kHeads, 1, 1});
    }
  }
  add("frontend.featurizer.weights", {kLayers + 1});
}

// WavLM relative-position bucket of d = key - query (num_buckets 320, max_distance 800,
// bidirectional): 160 per sign (d > 0: +160), |d| < 80 exact, then 80 log-spaced up to 159.
static int wavlm_rel_bucket(int d) {
  const int n = kRelBuckets / 2, exact = n / 2;
  const int r = std::abs(d);
  const int b = d > 0 ? n : 0;
  if (r < exact) return b + r;
  const int big = exact + (int)(std::log((double)r / exact) / std::log((double)kRelMaxDist / exact) * (n - exact));
  return b + std::min(big, n - 1);
}

void Hubert::finalize() {
  h_conv0_w = dev.upload(P(hp("feature_extractor.conv_layers.0.0.weight")));
  h_gn_g = dev.upload(P(hp("feature_extractor.conv_layers.0.2.weight")));
  h_gn_b = dev.upload(P(hp("feature_extractor.conv_layers.0.2.bias")));
  for (int i = 1; i < 7; ++i)
    h_conv[i] = pack_conv(P(hp("feature_extractor.conv_layers." + std::to_string(i) + ".0.weight")), kConvDim,
                          kConvDim, kConvK[i], nullptr, "");
  h_ln0_g = dev.upload(P(hp("layer_norm.weight")));
  h_ln0_b = dev.upload(P(hp("layer_norm.bias")));
  h_proj = pack_conv(P(hp("post_extract_proj.weight")), kHidden, kConvDim, 1, P(hp("post_extract_proj.bias")).data(),
                     "");
  {
    // weight_norm(dim=2): w[o][i][k] = g[k] * v[o][i][k] / ||v[:, :, k]||  (f64), then the
    // grouped layout: output column g*64 + o' (o' < 48 real, 48..63 zero) reading the
    // 48 input channels of group g.
    const auto& g = P(hp("encoder.pos_conv.0.weight_g"));
    const auto& v = P(hp("encoder.pos_conv.0.weight_v"));
    const auto& bias = P(hp("encoder.pos_conv.0.bias"));
    std::vector<double> nrm(kPosK, 0.0);
    for (int o = 0; o < kHidden; ++o)
      for (int i = 0; i < kPosGin; ++i)
        for (int k = 0; k < kPosK; ++k) {
          const double x = v[((size_t)o * kPosGin + i) * kPosK + k];
          nrm[k] += x * x;
        }
    const int Np = kPosGroups * kPosGout;
    std::vector<float> w((size_t)Np * kPosGin * kPosK, 0.f), b(Np, 0.f);
    for (int o = 0; o < kHidden; ++o) {
      const int col = (o / kPosGin) * kPosGout + o % kPosGin;
      b[col] = bias[o];
      for (int i = 0; i < kPosGin; ++i)
        for (int k = 0; k < kPosK; ++k)
          w[((size_t)col * kPosGin + i) * kPosK + k] =
              (float)(g[k] * (double)v[((size_t)o * kPosGin + i) * kPosK + k] / std::sqrt(nrm[k]));
    }
    h_pos = pack_conv(w, Np, kPosGin, kPosK, b.data(), "");
  }
  h_enc_g = dev.upload(P(hp("encoder.layer_norm.weight")));
  h_enc_b = dev.upload(P(hp("encoder.layer_norm.bias")));
  h_layers.assign(kLayers, HLayer{});
  for (int l = 0; l < kLayers; ++l) {
    const std::string p = "encoder.layers." + std::to_string(l) + ".";
    HLayer& L = h_layers[l];
    // fused [q | k | v] projection: rows 0..767 q, 768.. k, 1536.. v
    std::vector<float> w((size_t)3 * kHidden * kHidden), b(3 * kHidden);
    const char* order[3] = {"q_proj", "k_proj", "v_proj"};
    for (int j = 0; j < 3; ++j) {
      const auto& wj = P(hp(p + "self_attn." + order[j] + ".weight"));
      const auto& bj = P(hp(p + "self_attn." + order[j] + ".bias"));
      std::copy(wj.begin(), wj.end(), w.begin() + (size_t)j * kHidden * kHidden);
      std::copy(bj.begin(), bj.end(), b.begin() + j * kHidden);
    }
    L.qkv = pack_conv(w, 3 * kHidden, kHidden, 1, b.data(), "");
    L.out = pack_conv(P(hp(p + "self_attn.out_proj.weight")), kHidden, kHidden, 1,
                      P(hp(p + "self_attn.out_proj.bias")).data(), "");
    L.fc1 = pack_conv(P(hp(p + "fc1.weight")), kFfn, kHidden, 1, P(hp(p + "fc1.bias")).data(), "");
    L.fc2 = pack_conv(P(hp(p + "fc2.weight")), kHidden, kFfn, 1, P(hp(p + "fc2.bias")).data(), "");
    L.ln1_g = dev.upload(P(hp(p + "self_attn_layer_norm.weight")));
    L.ln1_b = dev.upload(P(hp(p + "self_attn_layer_norm.bias")));
    {
      // fc1 on LN1's input u: fc1(LN1(u)) = (u W'^T - mu cs) rstd + b + W beta, W' = W diag(gamma)
      const auto& w1 = P(hp(p + "fc1.weight"));
      const auto& b1 = P(hp(p + "fc1.bias"));
      const auto& g1 = P(hp(p + "self_attn_layer_norm.weight"));
      const auto& be1 = P(hp(p + "self_attn_layer_norm.bias"));
      std::vector<float> wf(w1.size()), bf(kFfn), cs(kFfn);
      for (int n = 0; n < kFfn; ++n) {
        double bb = b1[n], c = 0.0;
        for (int k = 0; k < kHidden; ++k) {
          const float wv = w1[(size_t)n * kHidden + k];
          wf[(size_t)n * kHidden + k] = wv * g1[k];
          bb += (double)wv * be1[k];
          const float x = wf[(size_t)n * kHidden + k];
          const uint16_t h = pack::f2bf(x);
          c += (double)pack::bf2f(h) + (double)pack::bf2f(pack::f2bf(x - pack::bf2f(h)));
        }
        bf[n] = (float)bb;
        cs[n] = (float)c;
      }
      L.fc1f = pack_conv(wf, kFfn, kHidden, 1, bf.data(), "");
      L.fc1_cs = dev.upload(cs);
    }
    L.ln2_g = dev.upload(P(hp(p + "final_layer_norm.weight")));
    L.ln2_b = dev.upload(P(hp(p + "final_layer_norm.bias")));
    if (wavlm) {
      // the gate reads grep_linear's 8 outputs only as sum(p[0:4]) and sum(p[4:8]): two dot products
      // with the summed rows (f64)
      const auto& gw = P(hp(p + "self_attn.grep_linear.weight"));
      const auto& gb = P(hp(p + "self_attn.grep_linear.bias"));
      const auto& ga = P(hp(p + "self_attn.grep_a"));
      const int dh = kHidden / kHeads;
      std::vector<float> pk(2 * dh + 2 + kHeads);
      for (int half = 0; half < 2; ++half) {
        double bs = 0.0;
        for (int j = 0; j < 4; ++j) bs += gb[4 * half + j];
        pk[2 * dh + half] = (float)bs;
        for (int c = 0; c < dh; ++c) {
          double ws = 0.0;
          for (int j = 0; j < 4; ++j) ws += gw[(size_t)(4 * half + j) * dh + c];
          pk[half * dh + c] = (float)ws;
        }
      }
      for (int h = 0; h < kHeads; ++h) pk[2 * dh + 2 + h] = ga[h];
      L.gate_w = dev.upload(pk);
    }
  }
  if (wavlm) {
    // bias[h][d + 778] = weight[bucket(d)][h]; the bucket is constant past either end
    static_assert(kAttnRelMax == 778 && kRelBuckets == 320 && kRelMaxDist == 800, "table range follows the buckets");
    const auto& rw = P(hp("encoder.layers.0.self_attn.relative_attention_bias.weight"));
    std::vector<float> tab((size_t)kHeads * kAttnRelStride, 0.f);
    for (int d = -kAttnRelMax; d <= kAttnRelMax; ++d) {
      const int bk = wavlm_rel_bucket(d);
      for (int h = 0; h < kHeads; ++h) tab[(size_t)h * kAttnRelStride + d + kAttnRelMax] = rw[(size_t)bk * kHeads + h];
    }
    h_rel_tab = dev.upload(tab);
  }
  // Featurizer weights: softmax over the 13 hidden states (s3prl Featurizer,
  // normalize=False), or a one-hot pick for `layer != -1` (s3prl.py:84-87).
  const auto& fw = P("frontend.featurizer.weights");
  h_fw.assign(kLayers + 1, 0.f);
  if (opt.layer >= 0) {
    h_fw[opt.layer] = 1.f;
  } else {
    double mx = fw[0], sum = 0.0;
    for (float x : fw) mx = std::max(mx, (double)x);
    for (float x : fw) sum += std::exp((double)x - mx);
    for (int i = 0; i <= kLayers; ++i) h_fw[i] = (float)(std::exp((double)fw[i] - mx) / sum);
  }
}

// Host-side plan of one (uniform or ragged) batch: frames per conv level,
// feature-extractor chunks whose conv0 output stays below 2 GiB (32-bit buffer
// offsets; 33 MB per 5 s utterance), and the int32 offset tables the kernels
// read (uploaded into the workspace).
HubertPlan Hubert::plan(int B, const int* lens) const {
  HubertPlan pl;
  pl.B = B;
  std::vector<int> T[7], Tout(B);
  for (int k = 0; k < 7; ++k) T[k].resize(B);
  for (int b = 0; b < B; ++b) {
    WSP_CHECK(lens[b] >= 1, "HuBERT needs at least 1 sample per utterance");
    // s3prl S3PRLUpstream.forward (MIN_SECOND = 0.05): an utterance shorter than
    // 800 samples runs zero-padded to 800 (conv0 reads zeros past the real
    // samples, and its GroupNorm statistics cover the padded frames); the
    // output keeps len(range(0, W, 320)) frames of the real length W (the
    // featurizer's length match trims the extra frame).
    int t = std::max(lens[b], kMinSamples);
    for (int k = 0; k < 7; ++k) T[k][b] = t = (t - kConvK[k]) / kConvS[k] + 1;
    Tout[b] = (lens[b] + kDownsample - 1) / kDownsample;
  }
  const size_t cap = kOperandCap / (kConvDim * sizeof(float));  // conv0 rows per chunk
  for (int b0 = 0; b0 < B;) {
    size_t rows = 0;
    int b1 = b0;
    while (b1 < B && (b1 == b0 || rows + T[0][b1] <= cap)) rows += T[0][b1++];
    pl.chunks.push_back({b0, b1});
    b0 = b1;
  }
  // offsets: global [seg6 | fseg | seg3 | seg4 | seg5], then per chunk [wseg | seg0 .. seg6] relative to the chunk
  auto prefix = [&](const std::vector<int>& v, int lo, int hi) {
    long long acc = 0;
    pl.offs.push_back(0);
    for (int b = lo; b < hi; ++b) {
      acc += v[b];
      WSP_CHECK(acc < (1LL << 31), "HuBERT batch too large");
      pl.offs.push_back((int)acc);
    }
    return (size_t)acc;
  };
  pl.M = prefix(T[6], 0, B);
  pl.Mout = prefix(Tout, 0, B);
  // CNN layers 4..6 run once over the whole batch when the level-3 rows fit a 2 GiB operand (r5:
  // the per-chunk launches of these short layers filled 112-446 of the 256 CUs)
  pl.M3 = prefix(T[3], 0, B);
  pl.M4 = prefix(T[4], 0, B);
  pl.M5 = prefix(T[5], 0, B);
  std::vector<int> lv(lens, lens + B);
  for (auto& c : pl.chunks) {
    c.off = pl.offs.size();
    c.samples = prefix(lv, c.b0, c.b1);
    for (int k = 0; k < 7; ++k) c.rows[k] = prefix(T[k], c.b0, c.b1);
    c.row6 = 0;
    for (int b = 0; b < c.b0; ++b) c.row6 += T[6][b];
    c.row3 = 0;
    for (int b = 0; b < c.b0; ++b) c.row3 += T[3][b];
    c.sample0 = 0;
    for (int b = 0; b < c.b0; ++b) c.sample0 += lens[b];
    c.maxT0 = *std::max_element(T[0].begin() + c.b0, T[0].begin() + c.b1);
    pl.maxA = std::max(pl.maxA, c.rows[0]);
    pl.maxB = std::max(pl.maxB, c.rows[1]);
    pl.maxChunk = std::max(pl.maxChunk, c.b1 - c.b0);
    pl.maxStats = std::max(pl.maxStats, hubert_conv0_stats_doubles(c.b1 - c.b0, c.maxT0));
  }
  pl.maxT6 = *std::max_element(T[6].begin(), T[6].end());
  // layers 4..6 batch-wide: more than one chunk, level-3 rows within a 2 GiB operand, and the
  // chunk buffers (free after the chunk loop) large enough for the level-4 / level-5 rows
  pl.tail_batch = opt.tail_batch && pl.chunks.size() > 1 && pl.M3 * kConvDim * sizeof(float) < kOperandCap &&
                  pl.M4 <= pl.maxA && pl.M5 <= pl.maxB;
  WSP_CHECK(pl.M * kFfn * sizeof(float) < ((size_t)1 << 31) - 64,
            "HuBERT batch too large for one call (frames * 3072 floats must stay below 2 GiB)");
  return pl;
}

namespace {
struct HubertWs {
  float *cnnA, *cnnB;  // feature-extractor ping-pong of the largest chunk
  double* stats;       // conv0 partial moments (f64)
  float *x, *x1, *qkv, *ao, *ffn;
  int* dseg;    // the plan's int32 offset tables
  float* lnst;  // LN1 row statistics: [M][6] (mean, M2) of 128-column pieces
  float* cnn3;  // tail_batch: [M3][512] level-3 rows of the whole batch
  float* gate;  // WavLM: [M][12] gate of the layer in flight
  size_t floats;
};
HubertWs hubert_ws(const HubertPlan& pl, bool wavlm, float* base) {
  const size_t M = pl.M;
  WsCursor c{base};
  HubertWs w;
  w.cnnA = c.take(pl.maxA * kConvDim);
  w.cnnB = c.take(pl.maxB * kConvDim);
  w.stats = reinterpret_cast<double*>(c.take(2 * pl.maxStats));
  w.x = c.take(M * kHidden);
  w.x1 = c.take(M * kHidden);
  w.qkv = c.take(M * 3 * kHidden);
  w.ao = c.take(M * kHidden);
  w.ffn = c.take(M * kFfn);
  w.dseg = reinterpret_cast<int*>(c.take(pl.offs.size()));
  w.lnst = c.take(M * (kHidden / 128) * 2);
  w.cnn3 = c.take(pl.tail_batch ? pl.M3 * kConvDim : 0);
  w.gate = c.take(wavlm ? M * kHeads : 0);
  w.floats = c.off;
  return w;
}
}  // namespace

size_t Hubert::ws_bytes(const HubertPlan& pl) const {
  return (hubert_ws(pl, wavlm, nullptr).floats * sizeof(float) + 255) & ~size_t(255);
}

void Hubert::forward(const float* wav, const HubertPlan& pl, float* feats, int cmn, float* ws, hipStream_t s) {
  const HubertWs W = hubert_ws(pl, wavlm, ws);
  float *cnnA = W.cnnA, *cnnB = W.cnnB, *x = W.x, *x1 = W.x1, *qkv = W.qkv, *ao = W.ao, *ffn = W.ffn;
  double* stats = W.stats;
  float* cnn6 = qkv;  // [M][512] CNN output of the whole batch; qkv is first written by layer 0
  float* pc = ffn;  // the pos_conv output is consumed before fc1 writes
  int* dseg = W.dseg;
  float *lnst = W.lnst, *cnn3 = W.cnn3, *gate = W.gate;
  // pageable source: the copy is staged before hipMemcpyAsync returns, so pl.offs may go away
  WSP_HIP(hipMemcpyAsync(dseg, pl.offs.data(), pl.offs.size() * sizeof(int), hipMemcpyHostToDevice, s));
  const int B = pl.B;
  const int M = (int)pl.M;
  const int* seg6 = dseg;           // [B+1] hidden-state rows per utterance
  const int* fseg = dseg + B + 1;   // [B+1] output feature rows per utterance
  const int* gseg3 = dseg + 2 * (B + 1);  // [B+1] batch-wide rows of conv levels 3, 4, 5
  const int* gseg4 = dseg + 3 * (B + 1);
  const int* gseg5 = dseg + 4 * (B + 1);

  auto conv = [&](const char* tag, const ConvW& cw, const float* a, int lda, float* out, int ldo, int rows, int Ti,
                  int stride, int pad, int act, const float* res, bool bias, const int* oseg, const int* iseg, int nseg,
                  int gcols = 0, int gcin = 0, const ConvGemmArgs* lnf = nullptr) {
    ConvGemmArgs g = lnf ? *lnf : ConvGemmArgs{};  // lnf carries the LayerNorm fold fields only
    one_operand(g, a, lda, cw.cin);
    // taps == 1 projections pass oseg null: row-local, no utterance structure needed
    fill(g, cw, rows, 1, 1, pad, out, ldo, act, nullptr, bias, oseg, nseg);
    g.stride = stride;
    g.Ti = oseg ? Ti : 1;  // row-local (taps 1) GEMMs: uniform T = Ti = 1 so input row == output row
    g.res = res;
    g.ldres = res ? ldo : 0;
    g.gcols = gcols;
    g.gcin = gcin;
    g.iseg = iseg;
    // x3_variant 5 only: the long-K / GELU GEMMs (CNN, fc1, fc2) on the 16x16x32 form of the 256 x 256
    // tile (r3 A/B: CNN -2 %, fc1 -3 %, fc2 -6 % per launch), QKV / out_proj on 32x32.  Under the
    // default 7 (and 8) every one of these GEMMs (N % 256 == 0) takes the LDS-DMA 16x16x32 tile, which
    // is faster than the register-staged 16x16x32 tile for QKV and out_proj too (tools/gemm_check,
    // profiles/r5a_gemm_check.txt: qkv / out_proj / fc1 / fc2 / cnn.c1 per launch, families 6 vs 7)
    const bool mf16 = opt.x3_variant == 5 && (std::strncmp(tag, "h_cnn", 5) == 0 || std::strcmp(tag, "h_fc1") == 0 ||
                                          std::strcmp(tag, "h_fc2") == 0);
    run(tag, 2.0 * rows * (gcols ? (double)cw.N * kPosGin / kPosGout : cw.N) * cw.K, s, [&] {
      if (opt.precision == 1)
        launch_conv_gemm_x3(g, cw.whi, cw.wlo, mf16 ? 6 : opt.x3_variant, s);
      else
        launch(g, cw, s);
    });
  };
  auto ln = [&](const char* tag, const float* in, const float* add, float* out, int rows, int D, const float* gm,
                const float* bt, int layer) {
    LayerNormArgs a{};
    a.x = in;
    a.ldx = D;
    a.add = add;
    a.ldadd = kPosGroups * kPosGout;
    a.gin = kPosGin;
    a.gout = kPosGout;
    a.gamma = gm;
    a.beta = bt;
    a.eps = 1e-5f;
    a.out = out;
    a.ldo = D;
    a.M = rows;
    a.D = D;
    if (layer >= 0 && (h_fw[layer] != 0.f || (opt.layer < 0 && layer == 0))) {
      // weighted mode initialises at hidden state 0; one-hot mode at the chosen one
      a.feat = feats;
      a.feat_w = h_fw[layer];
      a.feat_init = (opt.layer >= 0 || layer == 0) ? 1 : 0;
      a.seg = seg6;
      a.fseg = fseg;
      a.nseg = B;
    }
    run(tag, 0, s, [&] { launch_layernorm(a, s); });
  };

  // ---- feature extractor, utterance chunks
  for (const HubertChunk& c : pl.chunks) {
    const int nb = c.b1 - c.b0;
    const int* cs = dseg + c.off;  // [wseg | seg0 .. seg6], each nb+1, relative to the chunk
    auto lvl = [&](int k) { return cs + (size_t)(k + 1) * (nb + 1); };
    run("h_conv0", 2.0 * c.rows[0] * kConvDim * 10, s, [&] {
      launch_hubert_conv0(wav + c.sample0, nb, 0, 0, c.maxT0, h_conv0_w, h_gn_g, h_gn_b, stats, cnnA, s, cs, lvl(0));
    });
    float* src = cnnA;
    float* dst = cnnB;
    // profiling sub-classes per layer: h_cnn.c<i>
    static const char* kCnn[7] = {"", "h_cnn.c1", "h_cnn.c2", "h_cnn.c3", "h_cnn.c4", "h_cnn.c5", "h_cnn.c6"};
    const int last = pl.tail_batch ? 3 : 6;
    for (int i = 1; i <= last; ++i) {
      // the last layer writes this chunk's rows of the whole batch's level-`last` output
      float* o = i == 6 ? cnn6 + c.row6 * kConvDim : i == last ? cnn3 + c.row3 * kConvDim : dst;
      conv(kCnn[i], h_conv[i], src, kConvDim, o, kConvDim, (int)c.rows[i], (int)c.rows[i - 1], kConvS[i], 0,
           kActGelu, nullptr, false, lvl(i), lvl(i - 1), nb);
      std::swap(src, dst);
    }
  }
  if (pl.tail_batch) {
    // layers 4..6 once over the whole batch (the chunk buffers are free now): cnn3 -> cnnA -> cnnB -> cnn6
    static const char* kCnnT[3] = {"h_cnn.c4", "h_cnn.c5", "h_cnn.c6"};
    const int* gs[4] = {gseg3, gseg4, gseg5, seg6};
    const float* in = cnn3;
    float* outs[3] = {cnnA, cnnB, cnn6};
    const size_t rows[4] = {pl.M3, pl.M4, pl.M5, pl.M};
    for (int i = 4; i < 7; ++i) {
      conv(kCnnT[i - 4], h_conv[i], in, kConvDim, outs[i - 4], kConvDim, (int)rows[i - 3], (int)rows[i - 4], kConvS[i],
           0, kActGelu, nullptr, false, gs[i - 3], gs[i - 4], B);
      in = outs[i - 4];
    }
  }
  // LayerNorm + feature projection once over every chunk's rows (row-local: the same results as
  // per chunk, in one launch each instead of one per chunk with a few hundred blocks)
  ln("h_ln", cnn6, nullptr, cnn6, M, kConvDim, h_ln0_g, h_ln0_b, -1);
  conv("h_proj", h_proj, cnn6, kConvDim, x, kHidden, M, M, 1, 0, kActNone, nullptr, true, nullptr, nullptr, 0);
  // ---- encoder: x + GELU(pos_conv(x)) -> LN  (SamePad: pad 64, last output dropped)
  if (opt.precision == 1 && opt.pos_conv) {
    // direct grouped conv over the same packed weights (pos_conv.hip): 48 of 64 columns per group
    // computed, input patch split once per block
    run("h_pos_conv", 2.0 * M * kHidden * (double)h_pos.K, s, [&] {
      launch_hubert_pos_conv(x, kHidden, seg6, B, pl.maxT6, M, h_pos.whi, h_pos.wlo, h_pos.Kp, kPosGout, h_pos.bias,
                             pc, kPosGroups * kPosGout, s);
    });
  } else {
    conv("h_pos_conv", h_pos, x, kHidden, pc, kPosGroups * kPosGout, M, M, 1, kPosK / 2, kActGelu, nullptr, true,
         seg6, nullptr, B, kPosGout, kPosGin);
  }
  ln("h_ln", x, pc, x, M, kHidden, h_enc_g, h_enc_b, 0);
  // LayerNorm fold: the GEMMs it touches run on tile family 7 (x3_variant 7, bf16x3)
  const bool fold = opt.ln_fold && opt.precision == 1 && opt.x3_variant == 7;
  for (int l = 0; l < kLayers; ++l) {
    const HLayer& L = h_layers[l];
    conv("h_qkv", L.qkv, x, kHidden, qkv, 3 * kHidden, M, M, 1, 0, kActNone, nullptr, true, nullptr, nullptr, 0);
    AttnBias ab{h_rel_tab, gate};
    if (wavlm)  // the gate comes from the layer input x, not from q
      run("h_gate", 4.0 * M * kHidden, s, [&] { launch_attn_gate(x, kHidden, M, kHeads, L.gate_w, gate, s); });
    run("h_attn", 4.0 * B * kHeads * (double)pl.maxT6 * pl.maxT6 * (kHidden / kHeads), s, [&] {
      launch_attn(qkv, 3 * kHidden, ao, kHidden, B, pl.maxT6, kHeads, kHidden / kHeads, s, seg6, opt.attn_pipe,
                  wavlm ? &ab : nullptr);
    });
    if (fold) {
      // LN1 folded: out_proj emits x1's row statistics, fc1 runs on x1 with gamma1 / beta1 in its
      // weights, fc2 normalises its residual x1 on the fly (in place: each element is read by the
      // lane that then overwrites it)
      ConvGemmArgs f{};
      f.ln_parts = kHidden / 128;
      f.ln_eps = 1e-5f;
      f.lnmode = 1;
      f.ln_out = lnst;
      conv("h_out_proj", L.out, ao, kHidden, x1, kHidden, M, M, 1, 0, kActNone, x, true, nullptr, nullptr, 0, 0, 0, &f);
      f.lnmode = 2;
      f.ln_out = nullptr;
      f.ln_in = lnst;
      f.ln_cs = L.fc1_cs;
      conv("h_fc1", L.fc1f, x1, kHidden, ffn, kFfn, M, M, 1, 0, kActGelu, nullptr, true, nullptr, nullptr, 0, 0, 0, &f);
      f.lnmode = 4;
      f.ln_cs = nullptr;
      f.ln_g = L.ln1_g;
      f.ln_b = L.ln1_b;
      conv("h_fc2", L.fc2, ffn, kFfn, x1, kHidden, M, M, 1, 0, kActNone, x1, true, nullptr, nullptr, 0, 0, 0, &f);
    } else {
      conv("h_out_proj", L.out, ao, kHidden, x1, kHidden, M, M, 1, 0, kActNone, x, true, nullptr, nullptr, 0);
      ln("h_ln", x1, nullptr, x, M, kHidden, L.ln1_g, L.ln1_b, -1);
      conv("h_fc1", L.fc1, x, kHidden, ffn, kFfn, M, M, 1, 0, kActGelu, nullptr, true, nullptr, nullptr, 0);
      conv("h_fc2", L.fc2, ffn, kFfn, x1, kHidden, M, M, 1, 0, kActNone, x, true, nullptr, nullptr, 0);
    }
    ln("h_ln", x1, nullptr, x, M, kHidden, L.ln2_g, L.ln2_b, l + 1);
  }
  if (cmn) run("h_cmn", 0, s, [&] { launch_cmn_rows(feats, B, 0, kHidden, s, fseg); });
}

// ------------------------------------------------------------ Model API ---
bool Model::is_frontend() const { return impl->is_frontend(); }

int Model::out_frames(int N) const {
  as_hubert(impl, "out_frames: not a front-end handle");
  WSP_CHECK(N >= 1, "HuBERT needs at least 1 sample");
  return (N + kDownsample - 1) / kDownsample;
}

size_t Model::frontend_workspace_bytes(int B, int N) const {
  as_hubert(impl, "frontend_workspace_bytes: not a front-end handle");
  WSP_CHECK(B > 0 && N >= 1, "HuBERT needs B >= 1 and N >= 1 samples");
  const std::vector<int> lens(B, N);
  return frontend_workspace_bytes_segments(B, lens.data());
}

size_t Model::frontend_workspace_bytes_segments(int B, const int* lens) const {
  const Hubert& m = as_hubert(impl, "frontend_workspace_bytes: not a front-end handle");
  WSP_CHECK(B > 0 && lens, "HuBERT needs B >= 1 utterances");
  const int ns = m.nsub(B);
  size_t bytes = 256;
  for (int i = 0; i < ns; ++i) bytes += m.ws_bytes(m.plan(B * (i + 1) / ns - B * i / ns, lens + B * i / ns));
  return bytes;
}

void Model::forward_frontend(const float* wav, int B, int N, float* feats, int cmn, void* ws, size_t ws_bytes,
                             hipStream_t s) {
  WSP_CHECK(B > 0 && N >= 1, "HuBERT needs B >= 1 and N >= 1 samples");
  const std::vector<int> lens(B, N);
  forward_frontend_segments(wav, B, lens.data(), feats, nullptr, cmn, ws, ws_bytes, s);
}

void Model::forward_frontend_segments(const float* wav, int B, const int* lens, float* feats, int* frame_offsets,
                                      int cmn, void* ws, size_t ws_bytes, hipStream_t s) {
  Hubert& m = as_hubert(impl, "forward_frontend: not a front-end handle");
  WSP_CHECK(m.finalized, "forward before finalize");
  WSP_CHECK(B > 0 && lens, "HuBERT needs B >= 1 utterances");
  WSP_CHECK(ws_bytes >= frontend_workspace_bytes_segments(B, lens), "workspace too small");
  // utterance ranges on concurrent streams (option "streams"); each range's plan is
  // relative to its first sample / output frame
  const int ns = m.nsub(B);
  std::vector<HubertPlan> pls(ns);
  for (int i = 0; i < ns; ++i) {
    const int b0 = B * i / ns, b1 = B * (i + 1) / ns;
    pls[i] = m.plan(b1 - b0, lens + b0);
  }
  if (frame_offsets) {
    frame_offsets[0] = 0;
    int b = 0;
    for (int i = 0; i < ns; ++i) {
      const HubertPlan& pl = pls[i];
      const int base = frame_offsets[b];
      for (int j = 1; j <= pl.B; ++j) frame_offsets[b + j] = base + pl.offs[pl.B + 1 + j];
      b += pl.B;
    }
  }
  char* wsb = reinterpret_cast<char*>((reinterpret_cast<uintptr_t>(ws) + 255) & ~uintptr_t(255));
  if (ns > 1) m.fork(s, ns);
  size_t sample0 = 0, frame0 = 0;
  for (int i = 0; i < ns; ++i) {
    const HubertPlan& pl = pls[i];
    m.forward(wav + sample0, pl, feats + frame0 * kHidden, cmn, reinterpret_cast<float*>(wsb), m.sub(s, i));
    wsb += m.ws_bytes(pl);
    for (int b = B * i / ns; b < B * (i + 1) / ns; ++b) sample0 += lens[b];
    frame0 += pl.Mout;
  }
  if (ns > 1) m.join(s, ns);
}

}  // namespace wsp
