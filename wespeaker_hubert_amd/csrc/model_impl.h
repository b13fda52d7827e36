// Internal: the Model::Impl runtime object.  Declarations only; the bodies live in one
// translation unit per model family (source map):
//   model.cpp         Model API, parameter intake, shared pack / GEMM helpers, stream fork / join
//   ecapa_model.cpp   ECAPA-TDNN
//   resnet_model.cpp  ResNet and SimAM-ResNet
//   hubert_model.cpp  HuBERT / WavLM front end
//   campplus_model.cpp  CAM++
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
#include "res2_chain.h"
#include "astp_fused.h"
#include "conv3x3_img.h"

namespace wsp {

namespace detail {

constexpr double kBnEps = 1e-5;

struct DevBuf {
  std::vector<void*> ptrs;
  ~DevBuf() {
    for (void* p : ptrs) (void)hipFree(p);
  }
  void* upload_u16(const std::vector<uint16_t>& v) {
    void* p = nullptr;
    WSP_HIP(hipMalloc(&p, std::max<size_t>(v.size(), 1) * sizeof(uint16_t)));
    ptrs.push_back(p);
    if (!v.empty()) WSP_HIP(hipMemcpy(p, v.data(), v.size() * sizeof(uint16_t), hipMemcpyHostToDevice));
    return p;
  }
  float* upload(const std::vector<float>& v) {
    void* p = nullptr;
    WSP_HIP(hipMalloc(&p, std::max<size_t>(v.size(), 1) * sizeof(float)));
    ptrs.push_back(p);
    if (!v.empty()) WSP_HIP(hipMemcpy(p, v.data(), v.size() * sizeof(float), hipMemcpyHostToDevice));
    return static_cast<float*>(p);
  }
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

// HuBERT batch plan (hubert_model.cpp): utterance ranges of the feature
// extractor, their row counts per conv level, and the int32 offset tables.
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

struct Model::Impl {
  std::string arch;
  bool ecapa = true;
  int C = 512;
  bool glob = false;
  int feat_dim = 80, embed_dim = 192;
  bool emb_bn = false, two_emb = false;
  std::vector<Param> params;
  std::map<std::string, int> idx;
  bool finalized = false;
  int device = 0;
  DevBuf dev;

  // ------------------------------------------------------------------ ECAPA (ecapa_model.cpp) --
  ConvW layer1;
  struct Block {
    ConvW c1, c3, res2[7];
    LinW se1, se2;
    // the 7 Res2Net convs packed for res2_chain.hip (one launch per block)
    void* r2w = nullptr;
    float *r2b = nullptr, *r2s = nullptr, *r2t = nullptr;
  } blk[3];
  int res2_fused = 1;  // 0: the 7-launch GEMM chain (A/B option "res2_fused")
  int res2_variant = 4;  // res2_chain.hip kernel variant (option "res2_variant"; 4 = halo-free strips, C2 1.48 -> 1.24 ms/step; c512 widths run 3)
  ConvW conv, pool1, pool2;
  // conv_cat on [out2, out3, g4 * h3_4]: out4 = out3 + g4 * h3_4, so W . [out2; out3; out4]
  // = W_a out2 + (W_b + W_c) out3 + W_c (g4 * h3_4) — the last SE block's residual pass
  // writes only g4 * h3_4 (no residual read) (option "cat_gate", default on)
  ConvW conv_g;
  int cat_gate = 1;
  // with cat_gate: the gate pass itself is folded into conv_cat, whose third A segment is h3_4
  // multiplied by g4 as its fragments are read (ConvGemmArgs::gate) — no g4 * h3_4 tensor is
  // written or read.  Effective where the GEMM takes a gate (bf16x3 tile family 7 on uniform
  // batches with T >= 256); everything else keeps the gate pass (option "gate_fold", default on)
  int gate_fold = 1;
  void* pool2_frag = nullptr;  // pool.linear2 in MFMA B-fragment order for astp_fused.hip
  // 0: linear2 GEMM + separate pooling kernel; 1: astp_fused.hip (option "astp_fused"; 256 channels
  // per block, att chunks two ahead in an LDS-DMA ring, W2 in VGPRs: C2 0.465 -> 0.31 ms)
  int astp_fused_on = 1;
  LinW pool1_ctx;
  LinW head;
  void build_ecapa_params();
  void pack_res2(Block& b, const std::string& p, int w);
  void finalize_ecapa();
  int ecapa_chunk(int B, int T) const;
  size_t ecapa_ws_floats(int B, size_t M) const;
  // seg (device [B+1] row offsets) non-null: ragged batch of M rows; T unused by the
  // kernels then (per-utterance lengths come from seg).
  void forward_ecapa(const float* feats, int B, int T, float* embed, float* ws, hipStream_t s,
                     const int* seg = nullptr, int M_seg = 0);

  // ----------------------------------------------- ResNet and SimAM-ResNet (resnet_model.cpp) --
  // ResNet (resnet.py:110-260), NHWC activations [B][F][T][C]
  bool bottleneck = true;
  int nblocks[4] = {0, 0, 0, 0};
  int m_ch = 32;
  float* stem_w = nullptr;
  float* stem_b = nullptr;
  // ResNet stride-1 3x3 convs on conv3x3_img.hip (option "conv3x3_img"): 0 = off (implicit GEMM),
  // 1 = 32 / 64 channels, 2 = also 128 channels (4 x 32 tile), 3 = also 128 (2 x 32 tile)
  int conv3x3_img_on = 2;
  int res_prefetch = 1;  // ResNet 1x1 residual convs: residual loaded ahead of the last k-tiles (option "res_prefetch")
  // ResNet bottleneck conv2 + conv3 (+ residual) of stride-1 blocks with planes 32 / 64 / 128 in one
  // launch, y2 kept in registers (conv3x3_img.hip bottleneck_tail; option "res_tail"): 1 = also the
  // next block's conv1 on the tail's output while it is on chip (tail2_kernel: two position runs
  // per wave), 2 = the tail alone, 0 = off
  int res_tail = 1;
  // bottleneck conv3 + projection shortcut fused: bit 0 as one GEMM (RBlock::c3sc), bit 1 inside
  // the fused tail (RBlock::w3scx)
  int sc_fuse = 3;
  int c1_stage_fuse = 1;  // a stage's first conv1 (4C -> 2C) inside the previous stage's last tail
  bool img_ok(const ConvW& cw, int C) const { return cw.frag && conv3x3_img_on && (C <= 64 || conv3x3_img_on >= 2); }
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
  // SimAM-ResNet (samresnet.py:20-166): basic blocks whose bn2 output passes
  // SimAM before the shortcut add, ASP pooling, `bottleneck` Linear.
  bool simam = false;
  ConvW asp1, asp2;
  LinW simam_head;
  struct RShapes {
    size_t big = 0, y1 = 0, y2 = 0, sc = 0;  // floats per utterance
    int F4 = 0, T4 = 0, C4 = 0;
  };
  void build_res_blocks(const std::string& pre, const char* sc_conv, const char* sc_bn);
  void build_resnet_params();
  void build_simam_params();
  ConvW pack_conv_bn(const std::string& wname, const std::string& bn, int N, int cin, int taps,
                     void** acc_frag = nullptr, void** b_frag = nullptr);
  void finalize_res_blocks(const std::string& pre, const char* sc_conv, const char* sc_bn);
  void finalize_resnet();
  void finalize_simam();
  RShapes resnet_shapes(int T) const;
  int resnet_chunk(int B, int T) const;
  size_t resnet_ws_floats(int B, int T) const;  // ResNet and SimAM-ResNet
  void gemm2d(const char* tag, const ConvW& cw, const float* a0, int lda, float* out, int ldo, int B, int Fi, int Ti,
              int kw, int stride, int pad, int act, const float* res, int ldres, hipStream_t s);
  void gemm1x1(const char* tag, const ConvW& cw, const float* a0, float* out, int M, int act, const float* res,
               hipStream_t s);
  void gemm_c3sc(const char* tag, const RBlock& rb, const float* y2, const float* x, int Ci, float* out, int B, int Fi,
                 int Ti, int Fo, int To, hipStream_t s);
  void conv3x3(const char* tag, const ConvW& cw, const float* in, int ldin, float* out, int B, int Fi, int Ti,
               int stride, bool relu, const float* res, hipStream_t s);
  void forward_resnet(const float* feats, int B, int T, float* embed, float* ws, hipStream_t s);
  void forward_simam(const float* feats, int B, int T, float* embed, float* ws, hipStream_t s);

  // ------------------------------------------------- HuBERT / WavLM front end (hubert_model.cpp) --
  // channels-last [B][T][C]
  bool hubert = false;
  float* h_conv0_w = nullptr;  // [512][10]
  float* h_gn_g = nullptr;
  float* h_gn_b = nullptr;
  ConvW h_conv[7];  // 1..6: strided feature-extractor convs (GELU epilogue)
  float* h_ln0_g = nullptr;
  float* h_ln0_b = nullptr;
  ConvW h_proj, h_pos;
  float* h_enc_g = nullptr;
  float* h_enc_b = nullptr;
  struct HLayer {
    ConvW qkv, out, fc1, fc2;
    float *ln1_g = nullptr, *ln1_b = nullptr, *ln2_g = nullptr, *ln2_b = nullptr;
    // LayerNorm fold (option ln_fold): fc1 on the un-normalised rows with gamma1 folded into W
    // and W beta1 into the bias; fc1_cs[n] = sum_c W'[n][c] (of the bf16 hi + lo images)
    ConvW fc1f;
    float* fc1_cs = nullptr;
    float* gate_w = nullptr;  // WavLM: [wa (64) | wb (64) | ba | bb | grep_a (12)] (attn.h launch_attn_gate)
  };
  // WavLM Base / Base+ (arch "WavLM_base"): HuBERT-base plus the gated relative-position bias
  bool wavlm = false;
  float* h_rel_tab = nullptr;  // [12][kAttnRelStride] bias per head over d = key - query in [-778, 778]
  std::vector<HLayer> h_layers;
  std::vector<float> h_fw;  // featurizer weight per hidden state
  int h_layer_sel = -1;     // s3prl `layer` (-1: softmax-weighted sum of all 13)
  int attn_pipe = 1;        // attn.hip: 1 = persistent pipelined kernel, 0 = one block per (utterance, head)
  int pos_conv = 1;         // HuBERT pos_conv: 1 = direct grouped conv (pos_conv.hip), 0 = grouped implicit GEMM
  // HuBERT: 1 = the post-attention LayerNorm folded into out_proj / fc1 / fc2 (x3_variant 7); measured
  // neutral on C4 (A/B 4 234 / 4 223 vs 4 233 / 4 232 emb/s, profiles/r5g_ln_fold.txt): default off
  int ln_fold = 0;
  // HuBERT CNN layers 4-6 once over the whole batch when the feature extractor runs in several
  // utterance chunks (r5); 0 = per chunk (the tests compare the two)
  int tail_batch = 1;
  void build_hubert_params();
  void finalize_hubert();
  int hubert_cnn_frames(int N, int upto) const;
  HubertPlan hubert_plan(int B, const int* lens) const;
  size_t hubert_ws_floats(const HubertPlan& pl) const;
  void forward_hubert(const float* wav, const HubertPlan& pl, float* feats, int cmn, float* ws, hipStream_t s);

  // ------------------------------------------------------------------ CAM++ (campplus_model.cpp) --
  // FCM head NHWC [B][F][T][32] (stem_w / stem_b as the ResNets'), then frame rows [B][T'][C]
  bool campp = false;
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
  // 1 = the dense layers' BN-ReLU inside the GEMM's A prologue; 0 = an elementwise pass of its own
  // into scratch (A/B runs only; option "cam_fused")
  int cam_fused = 1;
  void build_campp_params();
  void finalize_campp();
  int campp_chunk(int B, int T) const;
  size_t campp_ws_floats(int B, int T) const;
  void forward_campp(const float* feats, int B, int T, float* embed, float* ws, hipStream_t s);

  // ------------------------------------------------------------------- shared (model.cpp) --
  // 1 = bf16x3 split MFMA (default), 0 = exact f32 MFMA
  int precision = 1;
  // bf16x3 tile family (conv_gemm_x3.hip): 5 = 256 x 256 where N % 256 == 0, else 256 x 128;
  // 4 = 256 x 128; 3 = 128 x 128; 6 = 5 on 16x16x32 MFMAs; 7 = 6 with plain-epilogue GEMMs
  // staged by LDS-DMA (conv_gemm_x3_t6.hip) (option "x3_variant")
  int x3_variant = 5;

  // concurrent sub-batches (option "streams"): the batch's utterances are split
  // into `streams` contiguous ranges, each forwarded on its own HIP stream over its
  // own workspace slice, so one range's HBM-bound kernels run beside the other's
  // MFMA-bound GEMMs; the caller's stream forks to and joins them with events.
  int streams = 1;
  std::vector<hipStream_t> sub_st;  // streams 1.. (range 0 runs on the caller's stream)
  std::vector<hipEvent_t> sub_ev;   // [0] fork, [i] join of range i
  int nsub(int B) const { return std::max(1, std::min(streams, B)); }
  size_t ws_bytes_one(int B, int T) const;
  hipStream_t sub(hipStream_t s, int i) const { return i == 0 ? s : sub_st[i - 1]; }
  void fork(hipStream_t s, int ns);
  void join(hipStream_t s, int ns);

  // parameter table
  void add(const std::string& n, std::vector<int64_t> shape);
  void add_bn(const std::string& p, int64_t c);
  const std::vector<float>& P(const std::string& n) const;
  // eval BatchNorm as affine: y = x*scale + shift
  void bn_affine(const std::string& p, std::vector<double>& sc, std::vector<double>& sh) const;

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

}  // namespace wsp
