// Speaker-model runtime, the part every family shares: the Model API, parameter intake
// (reference state_dict order), pack-and-upload helpers (BatchNorm folding and packing run on
// the host in f64), the implicit-GEMM launch helpers, sub-batch streams, options and profiling.
// The families derive from Model::Impl: their tables, folds, workspace layouts and forward
// schedules are in ecapa_model.cpp, resnet_model.cpp (ResNet and SimAM-ResNet), hubert_model.cpp,
// campplus_model.cpp, eres2net_model.cpp, gemini_model.cpp, xvec_model.cpp, redimnet_model.cpp, res2net_model.cpp and repvgg_model.cpp; Model::create below is the one place here that names them.
#include "model_impl.h"

namespace wsp {

int detail::chunk_for(int B, size_t bytes) {
  const int bc = std::min((int)std::max<size_t>(1, kOperandCap / bytes), B);
  const int chunks = (B + bc - 1) / bc;
  return (B + chunks - 1) / chunks;
}

// ------------------------------------------------------ parameter table ---
void Model::Impl::add(const std::string& n, std::vector<int64_t> shape) {
  idx[n] = (int)params.size();
  params.push_back(Param{n, std::move(shape), {}, false});
}
void Model::Impl::add_bn(const std::string& p, int64_t c) {
  add(p + ".weight", {c});
  add(p + ".bias", {c});
  add(p + ".running_mean", {c});
  add(p + ".running_var", {c});
  add(p + ".num_batches_tracked", {});
}
const std::vector<float>& Model::Impl::P(const std::string& n) const {
  auto it = idx.find(n);
  WSP_CHECK(it != idx.end(), "missing parameter " + n);
  const Param& p = params[it->second];
  WSP_CHECK(p.set || p.numel() == 0, "parameter not set: " + n);
  return p.host;
}

void Model::Impl::bn_affine(const std::string& p, std::vector<double>& sc, std::vector<double>& sh) const {
  const auto& w = P(p + ".weight");
  const auto& b = P(p + ".bias");
  const auto& rm = P(p + ".running_mean");
  const auto& rv = P(p + ".running_var");
  sc.resize(w.size());
  sh.resize(w.size());
  for (size_t i = 0; i < w.size(); ++i) {
    sc[i] = (double)w[i] / std::sqrt((double)rv[i] + kBnEps);
    sh[i] = (double)b[i] - (double)rm[i] * sc[i];
  }
}

Model::Impl::Folded Model::Impl::fold_bn(const std::string& wname, const std::string& bn) const {
  std::vector<double> sc, sh;
  bn_affine(bn, sc, sh);
  Folded f{P(wname), std::vector<float>(sh.begin(), sh.end())};
  const size_t K = f.w.size() / sc.size();
  for (size_t i = 0; i < f.w.size(); ++i) f.w[i] = (float)(f.w[i] * sc[i / K]);
  return f;
}

// ------------------------------------------------------ pack and upload ---
ConvW Model::Impl::pack_conv(const std::vector<float>& w, int N, int cin, int taps, const float* bias,
                             const std::string& bn) {
  ConvW cw;
  cw.N = N;
  cw.cin = cin;
  cw.taps = taps;
  cw.K = cin * taps;
  cw.Kp = round_up(cw.K, 64);  // even number of 32-wide k-tiles (bf16x3 pipeline)
  const std::vector<float> packed = pack::conv_kmajor(w, N, cin, taps, cw.Kp);
  std::vector<uint16_t> hi, lo;
  pack::split(packed, hi, lo);
  cw.w = dev.upload(packed);
  cw.whi = dev.upload_u16(hi);
  cw.wlo = dev.upload_u16(lo);
  if (bias) cw.bias = dev.upload(std::vector<float>(bias, bias + N));
  if (!bn.empty()) {
    std::vector<double> sc, sh;
    bn_affine(bn, sc, sh);
    cw.scale = dev.upload(std::vector<float>(sc.begin(), sc.end()));
    cw.shift = dev.upload(std::vector<float>(sh.begin(), sh.end()));
  }
  return cw;
}

LinW Model::Impl::pack_lin(const float* w, int N, int K, int ldk, const float* bias) {
  LinW lw;
  lw.N = N;
  lw.K = K;
  lw.wt = dev.upload(pack::transpose(w, N, K, ldk));
  if (bias) lw.bias = dev.upload(std::vector<float>(bias, bias + N));
  return lw;
}

// -------------------------------------------------------------- launches ---
void Model::Impl::one_operand(ConvGemmArgs& g, const float* a, int lda, int cin) {
  g.a[0] = g.a[1] = g.a[2] = a;
  g.lda[0] = g.lda[1] = g.lda[2] = lda;
  g.cseg[0] = 0;
  g.cseg[1] = g.cseg[2] = g.cseg[3] = cin;
}

void Model::Impl::fill(ConvGemmArgs& g, const ConvW& cw, int M, int T, int dil, int pad, float* out, int ldo, int act,
                       const float* row_bias, bool use_bias, const int* seg, int nseg) {
  g.cin = cw.cin;
  g.taps = cw.taps;
  g.dil = dil;
  g.pad = pad;
  g.M = M;
  g.T = T;
  g.N = cw.N;
  g.w = cw.w;
  g.K = cw.K;
  g.Kp = cw.Kp;
  g.bias = use_bias ? cw.bias : nullptr;
  g.row_bias = row_bias;
  g.scale = cw.scale;
  g.shift = cw.shift;
  g.out = out;
  g.ldo = ldo;
  g.act = act;
  g.seg = seg;
  g.nseg = nseg;
}

void Model::Impl::launch(const ConvGemmArgs& g, const ConvW& cw, hipStream_t s) {
  if (opt.precision == 1)
    launch_conv_gemm_x3(g, cw.whi, cw.wlo, opt.x3_variant, s);
  else
    launch_conv_gemm(g, s);
}

void Model::Impl::gemm(const char* tag, const ConvW& cw, const float* a0, int lda, float* out, int ldo, int M, int T,
                       int dil, int pad, int act, hipStream_t s, const int* seg, int nseg, const float* row_bias,
                       bool use_bias, int role) {
  ConvGemmArgs g{};
  one_operand(g, a0, lda, cw.cin);
  g.role = role;
  fill(g, cw, M, T, dil, pad, out, ldo, act, row_bias, use_bias, seg, nseg);
  run(tag, 2.0 * M * cw.N * cw.K, s, [&] { launch(g, cw, s); });
}

// --------------------------------------------------- sub-batch streams ---
void Model::Impl::fork(hipStream_t s, int ns) {
  while ((int)sub_st.size() < ns - 1) {
    hipStream_t t;
    WSP_HIP(hipStreamCreateWithFlags(&t, hipStreamNonBlocking));
    sub_st.push_back(t);
  }
  while ((int)sub_ev.size() < ns) {
    hipEvent_t e;
    WSP_HIP(hipEventCreateWithFlags(&e, hipEventDisableTiming));
    sub_ev.push_back(e);
  }
  WSP_HIP(hipEventRecord(sub_ev[0], s));
  for (int i = 1; i < ns; ++i) WSP_HIP(hipStreamWaitEvent(sub_st[i - 1], sub_ev[0], 0));
}
void Model::Impl::join(hipStream_t s, int ns) {
  for (int i = 1; i < ns; ++i) {
    WSP_HIP(hipEventRecord(sub_ev[i], sub_st[i - 1]));
    WSP_HIP(hipStreamWaitEvent(s, sub_ev[i], 0));
  }
}

// ------------------------------------------------------------ Model API ---
Model::Impl::~Impl() {
  for (auto& kv : prof_map)
    for (auto& e : kv.second.ev) {
      (void)hipEventDestroy(e.first);
      (void)hipEventDestroy(e.second);
    }
  for (auto t : sub_st) (void)hipStreamDestroy(t);
  for (auto e : sub_ev) (void)hipEventDestroy(e);
}

Model::~Model() { delete impl; }

void Model::create(const std::string& arch, int feat_dim, int embed_dim, bool emb_bn, bool two_emb) {
  WSP_CHECK(!impl, "model already created");
  for (MakeImpl* make : {make_ecapa, make_resnet, make_hubert, make_campplus, make_eres2net, make_gemini, make_xvec,
                         make_redimnet, make_res2net, make_repvgg})
    if ((impl = make(arch, feat_dim, embed_dim, emb_bn, two_emb))) break;
  WSP_CHECK(impl, "unsupported arch " + arch);
  // Creation and parameter intake are host-only; the device is bound at
  // finalize (create's device when one was current).
  if (hipGetDevice(&impl->device) != hipSuccess) {
    (void)hipGetLastError();
    impl->device = -1;
  }
  impl->build_params();
}

int Model::num_params() const { return (int)impl->params.size(); }

void Model::param_info(int i, const char** name, int* ndim, int64_t* shape) const {
  WSP_CHECK(i >= 0 && i < num_params(), "param index out of range");
  const Param& p = impl->params[i];
  *name = p.name.c_str();
  *ndim = (int)p.shape.size();
  for (size_t d = 0; d < p.shape.size() && d < 4; ++d) shape[d] = p.shape[d];
}

void Model::set_param(int i, const float* data, int64_t numel) {
  WSP_CHECK(i >= 0 && i < num_params(), "param index out of range");
  Param& p = impl->params[i];
  WSP_CHECK(numel == p.numel(), "numel mismatch for " + p.name);
  p.host.assign(data, data + numel);
  p.set = true;
}

void Model::finalize() {
  Impl& m = *impl;
  WSP_CHECK(!m.finalized, "model already finalized");
  int dev = 0;
  WSP_HIP(hipGetDevice(&dev));
  WSP_CHECK(m.device < 0 || dev == m.device, "finalize on a different device than create");
  m.device = dev;
  for (auto& p : m.params)
    WSP_CHECK(p.set || p.name.find("num_batches_tracked") != std::string::npos,
              "parameter not set: " + p.name);
  m.finalize();
  for (auto& p : m.params) std::vector<float>().swap(p.host);
  m.finalized = true;
}

int Model::embed_dim() const { return impl->embed_dim; }
int Model::feat_dim() const { return impl->feat_dim; }

// one workspace slice per sub-batch, 256-byte granules
size_t Model::workspace_bytes(int B, int T) const {
  WSP_CHECK(!impl->is_frontend(), "HuBERT handle: use the front-end workspace query");
  const int ns = impl->nsub(B);
  size_t bytes = 256;
  for (int i = 0; i < ns; ++i) bytes += impl->ws_bytes_one(B * (i + 1) / ns - B * i / ns, T);
  return bytes;
}

void Model::forward(const float* feats, int B, int T, float* embed, void* ws, size_t ws_bytes,
                    hipStream_t s) {
  Impl& m = *impl;
  WSP_CHECK(!m.is_frontend(), "HuBERT handle: use the front-end forward");
  WSP_CHECK(m.finalized, "forward before finalize");
  if (m.min_frames() >= 2)
    WSP_CHECK(B > 0 && T > 1, "forward needs B >= 1 and T >= 2 frames");
  else  // XI pooling is defined on one frame (the prior is its second entry)
    WSP_CHECK(B > 0 && T >= 1, "forward needs B >= 1 and T >= 1 frames");
  WSP_CHECK((size_t)B * T < (1u << 31), "B*T too large");
  WSP_CHECK(ws_bytes >= workspace_bytes(B, T), "workspace too small");
  m.check_forward(B, T);
  char* wsb = reinterpret_cast<char*>((reinterpret_cast<uintptr_t>(ws) + 255) & ~uintptr_t(255));
  const int ns = m.nsub(B);
  if (ns > 1) m.fork(s, ns);
  for (int i = 0; i < ns; ++i) {
    const int b0 = B * i / ns, nb = B * (i + 1) / ns - b0;
    const float* f = feats + (size_t)b0 * T * m.feat_dim;
    float* e = embed + (size_t)b0 * m.embed_dim;
    m.forward(f, nb, T, e, reinterpret_cast<float*>(wsb), m.sub(s, i));
    wsb += m.ws_bytes_one(nb, T);
  }
  if (ns > 1) m.join(s, ns);
}

// Ragged batches: one launch sequence over all M rows (no chunking, no sub-batch streams).
size_t Model::workspace_bytes_segments(int B, int M) const {
  WSP_CHECK(impl->has_segments(), "segmented batches are implemented for ECAPA-TDNN handles");
  WSP_CHECK(B > 0 && M >= B, "segmented batch needs B >= 1 and M >= B rows");
  return impl->ws_floats_segments(B, M) * sizeof(float) + 256;
}

void Model::forward_segments(const float* feats, int B, const int* seg, int M, float* embed, void* ws,
                             size_t ws_bytes, hipStream_t s) {
  Impl& m = *impl;
  WSP_CHECK(m.has_segments(), "segmented batches are implemented for ECAPA-TDNN handles");
  WSP_CHECK(m.finalized, "forward before finalize");
  WSP_CHECK(seg != nullptr && B > 0 && M >= B, "segmented batch needs offsets, B >= 1 and M >= B rows");
  WSP_CHECK((size_t)M * 1536 < (1u << 31) / 4, "segmented batch too large");
  WSP_CHECK(ws_bytes >= workspace_bytes_segments(B, M), "workspace too small");
  float* wsf = reinterpret_cast<float*>((reinterpret_cast<uintptr_t>(ws) + 255) & ~uintptr_t(255));
  m.forward_segments(feats, B, seg, M, embed, wsf, s);
}

void Model::profile(bool on) {
  if (on && !impl->prof)  // a new profiling window: drop the previous one's launches
    for (auto& kv : impl->prof_map) {
      kv.second.used = 0;
      kv.second.flops = 0;
    }
  impl->prof = on;
}

// One table behind set_option and get_option: key, Options member, accepted range [lo, hi] without
// `hole`, and the refusal's message.
namespace {
struct Opt {
  const char* key;
  int Options::*field;
  int lo, hi, hole;
  const char* err;
};
using I = Options;
constexpr int kNoHole = -1000;
const Opt kOpts[] = {
    {"precision", &I::precision, 0, 1, kNoHole, "precision must be 0 (f32) or 1 (bf16x3)"},
    {"streams", &I::streams, 1, 8, kNoHole, "streams must be 1..8"},
    {"layer", &I::layer, -1, 12, kNoHole, "layer must be -1 (weighted sum) or 0..12"},
    {"in_planes", &I::in_planes, 32, 64, kNoHole, "in_planes must be 32 or 64"},  // the two ends only (set_option)
    {"res2_fused", &I::res2_fused, 0, 1, kNoHole, "res2_fused must be 0 or 1"},
    {"cam_fused", &I::cam_fused, 0, 1, kNoHole, "cam_fused must be 0 (separate BN-ReLU pass) or 1 (GEMM prologue)"},
    {"ib_fused", &I::ib_fused, 0, 1, kNoHole, "ib_fused must be 0 (conv1, depthwise conv, conv3) or 1 (conv1, fused tail)"},
    {"res2_tail", &I::res2_tail, 0, 2, kNoHole,
     "res2_tail must be 0 (3x3 conv, then conv3), 1 (fused tail where it measured faster) or 2 (fused tail everywhere)"},
    {"rsbb_taps", &I::rsbb_taps, 0, 2, kNoHole,
     "rsbb_taps must be 0 (dense 25-tap conv), 1 (17 live taps where it measured faster) or 2 (17 live taps everywhere)"},
    {"cat_gate", &I::cat_gate, 0, 1, kNoHole, "cat_gate must be 0 or 1"},
    {"gate_fold", &I::gate_fold, 0, 1, kNoHole, "gate_fold must be 0 or 1"},
    {"seam_fold", &I::seam_fold, 0, 1, kNoHole, "seam_fold must be 0 or 1"},
    {"res_prefetch", &I::res_prefetch, 0, 1, kNoHole, "res_prefetch must be 0 or 1"},
    {"res_tail", &I::res_tail, 0, 2, kNoHole, "res_tail must be 0 (off), 1 (tail + next conv1) or 2 (tail alone)"},
    {"sc_fuse", &I::sc_fuse, 0, 3, kNoHole, "sc_fuse must be 0 .. 3 (bit 0: one GEMM, bit 1: in the tail)"},
    {"c1_stage_fuse", &I::c1_stage_fuse, 0, 1, kNoHole, "c1_stage_fuse must be 0 or 1"},
    {"astp_fused", &I::astp_fused, 0, 3, kNoHole,
     "astp_fused must be 0 (linear2 GEMM + pooling kernel) or 1 (fused)"},
    {"attn_pipe", &I::attn_pipe, 0, 1, kNoHole, "attn_pipe must be 0 or 1"},
    {"pos_conv", &I::pos_conv, 0, 1, kNoHole,
     "pos_conv must be 0 (grouped implicit GEMM) or 1 (direct grouped conv)"},
    {"ln_fold", &I::ln_fold, 0, 1, kNoHole, "ln_fold must be 0 (LayerNorm kernels) or 1 (folded into the GEMMs)"},
    {"tail_batch", &I::tail_batch, 0, 1, kNoHole,
     "tail_batch must be 0 (CNN layers 4-6 per chunk) or 1 (batch-wide)"},
    {"res2_variant", &I::res2_variant, 0, 4, 1,
     "res2_variant must be 0 (4 waves, 2 x 2), 2 (4 waves on N, 4 W k-steps in flight), 3 (8 waves) "
     "or 4 (halo-free strips, c1024 widths; else as 3)"},
    {"x3_variant", &I::x3_variant, 0, 9, kNoHole,
     "x3_variant must be 3, 4, 5, 6 (5 on 16x16x32 MFMAs) or 7 (6 staged by LDS-DMA)"},
    {"conv3x3_img", &I::conv3x3_img, 0, 3, kNoHole,
     "conv3x3_img must be 0 (off), 1 (32 / 64 channels) or 2 / 3 (also 128)"},
};
const Opt& find_opt(const std::string& key) {
  for (const Opt& o : kOpts)
    if (key == o.key) return o;
  throw InvalidArg{"unknown option " + key};
}
}  // namespace

void Model::set_option(const std::string& key, int value) {
  Impl& m = *impl;
  // pruned in r3 (hubert.hip's streaming mha_kernel, conv1x1_rows.hip): accepted, no effect
  if (key == "attn_lds" || key == "conv1x1_rows") return;
  const Opt& o = find_opt(key);
  if (key == "layer") {
    WSP_CHECK(m.owns_option(key), "option 'layer' applies to the HuBERT front end");
    WSP_CHECK(!m.finalized, "option 'layer' must be set before finalize");
  } else if (key == "in_planes") {
    WSP_CHECK(m.owns_option(key), "option 'in_planes' applies to SimAM-ResNet handles");
    WSP_CHECK(!m.finalized, "option 'in_planes' must be set before finalize");
    WSP_CHECK(value == 32 || value == 64, o.err);
    for (const auto& p : m.params) WSP_CHECK(!p.set, "option 'in_planes' must be set before the weights");
  } else if (key == "res2_tail") {
    WSP_CHECK(m.owns_option(key), "option 'res2_tail' applies to Res2Net handles");
  } else if (key == "rsbb_taps") {
    WSP_CHECK(m.owns_option(key), "option 'rsbb_taps' applies to RepVGG handles");
  }
  WSP_CHECK(value >= o.lo && value <= o.hi && value != o.hole, o.err);
  if (key == "x3_variant") {
    // 0 / 1 (unswizzled tiles), 2 / 9 (the r2 LDS-DMA tiles): pruned in r3; 8 (the r5 ping-pong form
    // of 7, bit-identical and slower): pruned in r5 — deprecated aliases of 5 / 7
    value = value >= 3 && value <= 7 ? value : value == 8 ? 7 : 5;
  } else if (key == "astp_fused") {
    value = value ? 1 : 0;  // 2 / 3: former fused variants (r3 pruned), deprecated aliases of 1
  }
  m.opt.*o.field = value;
  if (key == "in_planes") m.build_params();  // the parameter table follows the stem width
}

int Model::get_option(const std::string& key) const { return impl->opt.*find_opt(key).field; }

void Model::profile_query(const std::string& tag, int* launches, double* total_ms, double* flops) {
  // `tag` names one kernel class or, as a prefix "tag.", every sub-class under it
  // (e.g. "res_conv1x1" = "res_conv1x1.c1.L1" + ...).  Launches of the current /
  // last profiling window.
  *launches = 0;
  *total_ms = 0;
  *flops = 0;
  double fl = 0;
  for (auto& kv : impl->prof_map) {
    const std::string& k = kv.first;
    if (k != tag && k.compare(0, tag.size() + 1, tag + ".") != 0) continue;
    ProfEntry& e = kv.second;
    for (size_t i = 0; i < e.used; ++i) {
      WSP_HIP(hipEventSynchronize(e.ev[i].second));
      float ms = 0;
      WSP_HIP(hipEventElapsedTime(&ms, e.ev[i].first, e.ev[i].second));
      *total_ms += ms;
    }
    *launches += (int)e.used;
    fl += e.flops;
  }
  *flops = *launches ? fl / (double)*launches : 0.0;
}

}  // namespace wsp
