// Internal: Model::Impl, the base every architecture family derives from.  It holds what the
// families share (model.cpp): the parameter table, pack-and-upload and GEMM launch helpers,
// sub-batch streams, options and profiling.  A family is one `final` subclass with its own
// state, defined in its own translation unit (source map and "adding a family"):
//   ecapa_model.cpp   Ecapa     resnet_model.cpp    ResNet (and SimAM-ResNet)
//   hubert_model.cpp  Hubert    campplus_model.cpp  Campplus
//   eres2net_model.cpp  Eres2Net  gemini_model.cpp  Gemini
//   xvec_model.cpp    Xvec (XVEC with TSTP, XI_VEC_XVEC with XI pooling)
//   redimnet_model.cpp  Redimnet (ReDimNetB2)   res2net_model.cpp  Res2Net
//   repvgg_model.cpp  RepVgg (RepVGG and RepSPK blocks, deploy form)
#pragma once

#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <algorithm>
#include <map>
#include <string>
#include <vector>

#include "kernels.h"
#include "model.h"
#include "pack.h"

namespace wsp {

namespace detail {

constexpr double kBnEps = 1e-5;

struct DevBuf {
  std::vector<void*> ptrs;
  ~DevBuf() {
    for (void* p : ptrs) (void)hipFree(p);
  }
  template <typename T>
  T* upload(const std::vector<T>& v) {
    void* p = nullptr;
    WSP_HIP(hipMalloc(&p, std::max<size_t>(v.size(), 1) * sizeof(T)));
    ptrs.push_back(p);
    if (!v.empty()) WSP_HIP(hipMemcpy(p, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice));
    return static_cast<T*>(p);
  }
  void* upload_u16(const std::vector<uint16_t>& v) { return upload(v); }
};

struct ConvW {
  float* w = nullptr;
  void* whi = nullptr;  // bf16 hi / lo split images for the bf16x3 kernel
  void* wlo = nullptr;
  float* bias = nullptr;
  float* scale = nullptr;
  float* shift = nullptr;
  int N = 0, cin = 0, taps = 1, K = 0, Kp = 0;
  void* frag = nullptr;  // MFMA B-fragment order of a stride-1 3x3 conv with N = cin (conv3x3_img.hip)
};

struct LinW {  // small_linear weights, k-major
  float* wt = nullptr;
  float* bias = nullptr;
  int K = 0, N = 0;
};

inline int round_up(int a, int b) { return (a + b - 1) / b * b; }

// Every activation operand of a kernel must stay below 2 GiB (32-bit buffer-load offsets): the
// chunk rules keep them within 7/8 of it.
constexpr size_t kOperandCap = ((size_t)1 << 31) / 8 * 7;
// Utterances per forward chunk of a batch of B whose widest operand takes `bytes` per utterance:
// the fewest chunks that respect kOperandCap, evenly sized.
int chunk_for(int B, size_t bytes);

// Workspace layout cursor: regions follow one another, each rounded up to 64 floats (256 B).
// A null base only measures (the workspace size queries); off is the running total.
struct WsCursor {
  float* base = nullptr;
  size_t off = 0;
  static size_t padded(size_t n) { return (n + 63) / 64 * 64; }
  float* take(size_t n) {
    float* p = base ? base + off : nullptr;
    off += padded(n);
    return p;
  }
};

}  // namespace detail

using namespace detail;

struct Param {
  std::string name;
  std::vector<int64_t> shape;
  std::vector<float> host;
  bool set = false;
  int64_t numel() const {
    int64_t n = 1;
    for (auto s : shape) n *= s;
    return n;
  }
};

struct ProfEntry {
  std::vector<std::pair<hipEvent_t, hipEvent_t>> ev;
  size_t used = 0;
  double flops = 0;
};

// The flat key space of wsp_model_set_option: every key reads and sets on every handle, whichever
// family consumes it.  Defaults here; create() sets the per-arch ones.
struct Options {
  int precision = 1;  // 1 = bf16x3 split MFMA, 0 = exact f32 MFMA
  // bf16x3 tile family (conv_gemm_x3.hip): 5 = 256 x 256 where N % 256 == 0, else 256 x 128;
  // 4 = 256 x 128; 3 = 128 x 128; 6 = 5 on 16x16x32 MFMAs; 7 = 6 with plain-epilogue GEMMs
  // staged by LDS-DMA (conv_gemm_x3_t6.hip)
  int x3_variant = 5;
  // concurrent sub-batches: the batch's utterances are split into `streams` contiguous ranges,
  // each forwarded on its own HIP stream over its own workspace slice, so one range's HBM-bound
  // kernels run beside the other's MFMA-bound GEMMs; the caller's stream forks to and joins them
  int streams = 1;
  // ECAPA-TDNN
  int res2_fused = 1;    // 0: the 7-launch GEMM chain
  int res2_variant = 4;  // res2_chain.hip kernel variant (4 = halo-free strips, C2 1.48 -> 1.24 ms/step; c512 widths run 3)
  // conv_cat on [out2, out3, g4 * h3_4]: out4 = out3 + g4 * h3_4, so W . [out2; out3; out4]
  // = W_a out2 + (W_b + W_c) out3 + W_c (g4 * h3_4) — the last SE block's residual pass
  // writes only g4 * h3_4 (no residual read)
  int cat_gate = 1;
  // with cat_gate: the gate pass itself is folded into conv_cat, whose third A segment is h3_4
  // multiplied by g4 as its fragments are read (ConvGemmArgs::gate) — no g4 * h3_4 tensor is
  // written or read.  Effective where the GEMM takes a gate (bf16x3 tile family 7 on uniform
  // batches with T >= 256); everything else keeps the gate pass
  int gate_fold = 1;
  // the first two blocks' x + g (.) h3 is formed by the next block's c1 as it stages its A operand
  // (ConvGemmArgs::seam_h, conv_gemm_x3_t7.hip) and written on the way: the residual pass is no
  // launch of its own.  Effective where the GEMM takes it (bf16x3 tile family 7 on uniform batches
  // with T >= 256); everything else keeps the pass
  int seam_fold = 1;
  // 0: linear2 GEMM + separate pooling kernel; 1: astp_fused.hip (256 channels per block, att
  // chunks two ahead in an LDS-DMA ring, W2 in VGPRs: C2 0.465 -> 0.31 ms)
  int astp_fused = 1;
  // ResNet and SimAM-ResNet
  int in_planes = 32;  // stem width (SimAM-ResNet: 64, settable before the weights)
  // stride-1 3x3 convs on conv3x3_img.hip: 0 = off (implicit GEMM), 1 = 32 / 64 channels,
  // 2 = also 128 channels (4 x 32 tile), 3 = also 128 (2 x 32 tile)
  int conv3x3_img = 2;
  int res_prefetch = 1;  // 1x1 residual convs: residual loaded ahead of the last k-tiles
  // bottleneck conv2 + conv3 (+ residual) of stride-1 blocks with planes 32 / 64 / 128 in one
  // launch, y2 kept in registers (conv3x3_img.hip bottleneck_tail): 1 = also the next block's
  // conv1 on the tail's output while it is on chip (tail2_kernel: two position runs per wave),
  // 2 = the tail alone, 0 = off
  int res_tail = 1;
  // bottleneck conv3 + projection shortcut fused: bit 0 as one GEMM (RBlock::c3sc), bit 1 inside
  // the fused tail (RBlock::w3scx)
  int sc_fuse = 3;
  int c1_stage_fuse = 1;  // a stage's first conv1 (4C -> 2C) inside the previous stage's last tail
  // HuBERT / WavLM front end
  int layer = -1;     // s3prl `layer` (-1: softmax-weighted sum of all 13)
  int attn_pipe = 1;  // attn.hip: 1 = persistent pipelined kernel, 0 = one block per (utterance, head)
  int pos_conv = 1;   // 1 = direct grouped conv (pos_conv.hip), 0 = grouped implicit GEMM
  // 1 = the post-attention LayerNorm folded into out_proj / fc1 / fc2 (x3_variant 7); measured
  // neutral on C4 (A/B 4 234 / 4 223 vs 4 233 / 4 232 emb/s, profiles/r5g_ln_fold.txt): default off
  int ln_fold = 0;
  // CNN layers 4-6 once over the whole batch when the feature extractor runs in several
  // utterance chunks (r5); 0 = per chunk (the tests compare the two)
  int tail_batch = 1;
  // CAM++: 1 = the dense layers' BN-ReLU inside the GEMM's A prologue; 0 = an elementwise pass of
  // its own into scratch (A/B runs only)
  int cam_fused = 1;
  // Gemini DF-ResNet: 0 = an inverted bottleneck is conv1, depthwise conv, projection as three
  // launches (the family's default: measured faster); 1 = conv1 + the fused tail (depthwise 3x3
  // inside the 1x1 projection's operand)
  int ib_fused = 0;
  // Res2Net: the tail of a block behind conv1 (3x3 conv of the first slice, conv3 over the
  // concatenation, residual).  0 = two launches (launch_eres_conv3x3, launch_eres_pw with ksplit);
  // 1 = one launch (res2net.hip) in the stages where it measured faster (res2net_model.cpp);
  // 2 = one launch in every stage (A/B runs)
  int res2_tail = 1;
  // RepVGG with RepSPK blocks (the *_RSBB_* names): the folded 5x5 conv of a block.  0 = all 25 taps
  // through the 2-D implicit GEMM; 2 = the 17 live taps (repvgg.hip) in every block whose eight dead taps
  // are zero; 1 = the 17 live taps in the stages where that measured faster (repvgg_model.cpp)
  int rsbb_taps = 1;
};

struct Model::Impl {
  std::string arch;
  int feat_dim = 80, embed_dim = 192;
  bool emb_bn = false, two_emb = false;
  Options opt;
  std::vector<Param> params;
  std::map<std::string, int> idx;
  bool finalized = false;
  int device = 0;
  DevBuf dev;

  Impl(const std::string& arch, int feat_dim, int embed_dim, bool emb_bn, bool two_emb)
      : arch(arch), feat_dim(feat_dim), embed_dim(embed_dim), emb_bn(emb_bn), two_emb(two_emb) {}
  virtual ~Impl();  // profiling events, sub-batch streams and their events

  // ---- what a family implements
  virtual void build_params() = 0;  // the parameter table, in the reference state_dict's order
  virtual void finalize() = 0;      // fold, pack and upload the weights
  // the family-specific keys ("layer", "in_planes") are refused on handles that do not own them
  virtual bool owns_option(const std::string&) const { return false; }
  // a front-end handle takes the wsp_frontend_* calls instead of forward / workspace_bytes
  virtual bool is_frontend() const { return false; }
  virtual void check_forward(int B, int T) const {}  // the family's forward preconditions
  virtual int min_frames() const { return 2; }  // the shortest uniform batch forward() takes at all
  // one sub-batch of B utterances of T frames (the family applies its own chunk rule inside)
  virtual size_t ws_floats(int B, int T) const = 0;
  virtual void forward(const float* feats, int B, int T, float* embed, float* ws, hipStream_t s) = 0;
  // ragged batches (ECAPA-TDNN, x-vector): utterance b = rows [seg[b], seg[b+1]) of M rows in all
  virtual bool has_segments() const { return false; }
  virtual size_t ws_floats_segments(int B, int M) const { return 0; }
  virtual void forward_segments(const float* feats, int B, const int* seg, int M, float* embed, float* ws,
                                hipStream_t s) {}

  // sub-batch streams (option "streams")
  std::vector<hipStream_t> sub_st;  // streams 1.. (range 0 runs on the caller's stream)
  std::vector<hipEvent_t> sub_ev;   // [0] fork, [i] join of range i
  int nsub(int B) const { return std::max(1, std::min(opt.streams, B)); }
  size_t ws_bytes_one(int B, int T) const { return (ws_floats(B, T) * sizeof(float) + 255) & ~size_t(255); }
  hipStream_t sub(hipStream_t s, int i) const { return i == 0 ? s : sub_st[i - 1]; }
  void fork(hipStream_t s, int ns);
  void join(hipStream_t s, int ns);

  // parameter table
  void add(const std::string& n, std::vector<int64_t> shape);
  void add_bn(const std::string& p, int64_t c);
  const std::vector<float>& P(const std::string& n) const;
  // eval BatchNorm as affine: y = x*scale + shift
  void bn_affine(const std::string& p, std::vector<double>& sc, std::vector<double>& sh) const;
  // conv -> eval BatchNorm folded into the conv: w[n][:] = W[n][:] * scale[n], b[n] = shift[n]
  struct Folded {
    std::vector<float> w, b;
  };
  Folded fold_bn(const std::string& wname, const std::string& bn) const;

  // pack (pack.h) and upload
  // Conv1d weight [N][cin][taps] -> packed [N][Kp], k = tap*cin + c; bn: its eval affine as scale / shift
  ConvW pack_conv(const std::vector<float>& w, int N, int cin, int taps, const float* bias, const std::string& bn);
  void* pack_frag(const std::vector<float>& w, int N, int K, pack::FragOrder order = pack::kPlain, int kacc = -1) {
    return dev.upload_u16(pack::frag(w, N, K, order, kacc));
  }
  void* pack_frag_acc(const std::vector<float>& w, int N, int K, int kacc = -1) { return pack_frag(w, N, K, pack::kAcc, kacc); }
  LinW pack_lin(const float* w, int N, int K, int ldk, const float* bias);

  // launches; seg / nseg: the segment table of a ragged batch (device row offsets [nseg + 1]) or null
  static void one_operand(ConvGemmArgs& g, const float* a, int lda, int cin);  // the three A slots on one tensor
  void fill(ConvGemmArgs& g, const ConvW& cw, int M, int T, int dil, int pad, float* out, int ldo, int act,
            const float* row_bias, bool use_bias, const int* seg, int nseg);
  void launch(const ConvGemmArgs& g, const ConvW& cw, hipStream_t s);
  void gemm(const char* tag, const ConvW& cw, const float* a0, int lda, float* out, int ldo, int M, int T, int dil,
            int pad, int act, hipStream_t s, const int* seg, int nseg, const float* row_bias = nullptr,
            bool use_bias = true, int role = 0);

  // profiling
  bool prof = false;
  std::map<std::string, ProfEntry> prof_map;
  template <typename F>
  void run(const char* tag, double flops, hipStream_t s, F&& f) {
    if (!prof) {
      f();
      return;
    }
    ProfEntry& e = prof_map[tag];
    if (e.used == e.ev.size()) {
      hipEvent_t a, b;
      WSP_HIP(hipEventCreate(&a));
      WSP_HIP(hipEventCreate(&b));
      e.ev.emplace_back(a, b);
    }
    auto& pr = e.ev[e.used++];
    e.flops += flops;  // summed; profile_query reports the mean per launch
    WSP_HIP(hipEventRecord(pr.first, s));
    f();
    WSP_HIP(hipEventRecord(pr.second, s));
  }
};

// One per family, defined beside its subclass: the arch names the family serves, their argument
// checks and per-arch option defaults.  Null: not one of that family's archs.
using MakeImpl = Model::Impl*(const std::string& arch, int feat_dim, int embed_dim, bool emb_bn, bool two_emb);
MakeImpl make_ecapa, make_resnet, make_hubert, make_campplus, make_eres2net, make_gemini, make_xvec, make_redimnet,
    make_res2net, make_repvgg;

}  // namespace wsp
