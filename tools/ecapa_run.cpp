// Op-level runner for ECAPA-TDNN's own kernels (tests/test_gpu_ecapa_op.py).
// Launches launch_res2_chain, launch_astp_fused, launch_astp_pool, launch_frame_stats,
// launch_small_linear, launch_residual_scale and, for the gated A tail and the SE-Res2Block seam,
// launch_conv_gemm_x3 of libwsp_hip.so, with the weights packed by the library's own
// pack::frag_res2 / pack::frag / pack::conv_kmajor + pack::split as the model packs them (small_linear's
// weight arrives k-major).  Framing, case and result files: tools/op_runner.h.  Magic 'WSPA' (0x41505357).  Arrays are
// f32; seg is i32 [B + 1] (row offsets of a ragged batch; an empty array where ragged = 0).  A header
// word called "f32" carries a float's bits.
//
//   op 1  res2_chain      hdr = w, variant, dil, B, T, M, ldx, ldo, ragged, rout_delta
//         arrays x [M][ldx], W [7][w][w][3] (torch layout), bias [7][w], scale [7][w], shift [7][w], seg
//         result out [(M + 8)][max(ldo, 7w)]: the launch gets row 4 as its first row, with
//         rout = res2_chain_rout(dil, variant, M) + rout_delta
//         own = rout as launched, CUs of the device
//   op 2  astp_fused      hdr = B, T, C, ldx, ragged, rows, var_floor (f32)
//         arrays att [rows][128], x [rows][ldx], W2 [C][128], bias2 [C], seg
//         result out [(B + 2)][2C]: the launch gets row 1
//   op 3  astp_pool       hdr = B, T, C, ragged, rows, eoff, var_floor (f32)
//         arrays e [eoff + rows C] (the launch gets the pointer eoff floats in: a view into a wider
//         upload), x [rows][C], seg
//         result out [(B + 2)][2C]: the launch gets row 1
//   op 4  frame_stats     hdr = B, T, C, ldx, ldo, with_std, std_off, ragged, rows
//         arrays x [rows][ldx], seg
//         result out [(B + 2)][ldo]: the launch gets row 1
//   op 5  small_linear    hdr = R, K, N, ldin, ldo, act, has_bias, scratch (0 none, 1 exactly
//                         small_linear_scratch_floats, 2 one float fewer offered)
//         arrays in [R][ldin], wt [K][N], bias [N] (or empty)
//         result out [(R + 2)][ldo]: the launch gets row 1
//   op 6  residual_scale  hdr = B, T, C, has_x, ragged, M
//         arrays x [M][C] (or empty), h [M][C], g [B][C], seg
//         result out [(M + 2)][C]: the launch gets row 1
//   op 7  gated A tail    hdr = variant, B, T, N, K, gate_k0, lda, ldg, ldo, ragged, M
//         arrays a [M][lda], w [N][K], bias [N], scale [N], shift [N], gate [B][ldg], seg
//         result out [(M + 8)][ldo]: the launch gets row 4
//         own = conv_gemm_x3_gate_ok's answer, 0
//   op 8  seam            hdr = variant, B, T, N, K, gate_k0, lda, ldg, ldo, ragged, M, ldh, ldso
//         arrays as op 7, then h [M][ldh]
//         results out [(M + 8)][ldo], seam_out [(M + 8)][ldso]: the launch gets row 4 of each
//         own = conv_gemm_x3_seam_ok's answer, 0
// Ops 7 / 8 are dense 1x1 GEMMs (one A segment, ReLU, scale / shift) through launch_conv_gemm_x3.
// Guard rows, and guard columns where a leading dimension exceeds the width, must come back untouched.
#include <algorithm>
#include <cstring>
#include <vector>

#include "../wespeaker_hubert_amd/csrc/astp_fused.h"
#include "../wespeaker_hubert_amd/csrc/kernels.h"
#include "../wespeaker_hubert_amd/csrc/pack.h"
#include "../wespeaker_hubert_amd/csrc/res2_chain.h"
#include "op_runner.h"

using namespace wsp;

namespace {

constexpr long long kMaxRows = 1 << 16;

float as_f32(int bits) {
  float f;
  std::memcpy(&f, &bits, 4);
  return f;
}

// the seg array of a case: B + 1 increasing offsets over `rows` rows when ragged, else empty
std::vector<int> offsets(Case& c, int ragged, int B, long long rows) {
  BAD(ragged == 0 || ragged == 1, "ragged must be 0 or 1");
  const std::vector<int> s = c.i32(ragged ? (long long)B + 1 : 0, "seg");
  if (ragged) {
    BAD(s[0] == 0 && s[B] == rows, "seg does not span the rows");
    for (int b = 0; b < B; ++b) BAD(s[b + 1] > s[b], "seg must increase (every utterance >= 1 frame)");
  }
  return s;
}

void run_res2(Case& c) {
  const int* h = c.h;
  const int w = h[0], variant = h[1], dil = h[2], B = h[3], T = h[4], M = h[5], ldx = h[6], ldo = h[7], ragged = h[8];
  BAD(w >= 32 && w <= 128 && w % 32 == 0 && variant >= 0 && variant <= 4 && dil >= 1 && dil <= 8, "res2: w / variant / dil");
  BAD(B >= 1 && B <= 4096 && T >= 1 && M >= 1 && M < kMaxRows && (ragged || M == (long long)B * T), "res2: batch");
  BAD(ldx >= 8 * w && ldx <= 2048 && ldo >= 1 && ldo <= 2048, "res2: leading dimensions");
  const auto x = c.f32((long long)M * ldx, "x");
  const auto W = c.f32((long long)7 * w * w * 3, "W");
  const auto bias = c.f32(7 * w, "bias"), scale = c.f32(7 * w, "scale"), shift = c.f32(7 * w, "shift");
  const auto seg = offsets(c, ragged, B, M);
  Pool& pool = c.pool;
  const int ldb = std::max(ldo, 7 * w);  // a row stride the launcher must refuse stays in bounds
  const size_t n = (size_t)(M + 8) * ldb;
  float* out = pool.filled(n);
  c.result(out, n);
  c.guarded([&] {
    c.own[1] = (uint32_t)device_cu_count();
    std::vector<float> Wi[7];
    const std::vector<float>* Wp[7];
    for (int i = 0; i < 7; ++i) {
      Wi[i].assign(W.begin() + (size_t)i * w * w * 3, W.begin() + (size_t)(i + 1) * w * w * 3);
      Wp[i] = &Wi[i];
    }
    Res2Args r{};
    r.x = pool.up(x);
    r.out = out + 4 * (size_t)ldb;
    r.ldx = ldx, r.ldo = ldo, r.M = M, r.T = T, r.dil = dil, r.variant = variant;
    r.rout = res2_chain_rout(dil, variant, M) + h[9];
    c.own[0] = (uint32_t)r.rout;
    if (ragged) r.seg = pool.up(seg), r.nseg = B;
    r.w = pool.up(pack::frag_res2(Wp, w));
    r.bias = pool.up(bias), r.scale = pool.up(scale), r.shift = pool.up(shift);
    launch_res2_chain(r, w, c.stream);
  });
}

void run_astp_fused(Case& c) {
  const int* h = c.h;
  const int B = h[0], T = h[1], C = h[2], ldx = h[3], ragged = h[4], rows = h[5];
  BAD(B >= 1 && B <= 64 && T >= 1 && T <= 4096 && C >= 32 && C <= 4096 && C % 32 == 0 && ldx >= C && ldx <= 8192,
      "astp_fused: shape");
  BAD(rows >= 1 && rows < kMaxRows && (ragged || rows == B * T), "astp_fused: rows");
  const auto att = c.f32((long long)rows * 128, "att"), x = c.f32((long long)rows * ldx, "x");
  const auto w2 = c.f32((long long)C * 128, "W2"), bias = c.f32(C, "bias2");
  const auto seg = offsets(c, ragged, B, rows);
  Pool& pool = c.pool;
  const size_t n = (size_t)(B + 2) * 2 * C;
  float* out = pool.filled(n);
  c.result(out, n);
  c.guarded([&] {
    AstpArgs a{pool.up(att), pool.up(x), ldx, B, T, C, ragged ? pool.up(seg) : nullptr,
               pool.up(pack::frag(w2, C, 128)), pool.up(bias), as_f32(h[6]), out + 2 * (size_t)C};
    launch_astp_fused(a, c.stream);
  });
}

void run_astp_pool(Case& c) {
  const int* h = c.h;
  const int B = h[0], T = h[1], C = h[2], ragged = h[3], rows = h[4], eoff = h[5];
  BAD(B >= 1 && B <= 64 && T >= 1 && T <= 4096 && C >= 1 && C <= 4096 && (eoff == 0 || eoff == 1), "astp_pool: shape");
  BAD(rows >= 1 && rows < kMaxRows && (ragged || rows == B * T), "astp_pool: rows");
  const auto e = c.f32((long long)eoff + (long long)rows * C, "e"), x = c.f32((long long)rows * C, "x");
  const auto seg = offsets(c, ragged, B, rows);
  Pool& pool = c.pool;
  const size_t n = (size_t)(B + 2) * 2 * C;
  float* out = pool.filled(n);
  c.result(out, n);
  c.guarded([&] {
    launch_astp_pool(pool.up(e) + eoff, pool.up(x), B, T, C, out + 2 * (size_t)C, c.stream,
                     ragged ? pool.up(seg) : nullptr, as_f32(h[6]));
  });
}

void run_frame_stats(Case& c) {
  const int* h = c.h;
  const int B = h[0], T = h[1], C = h[2], ldx = h[3], ldo = h[4], with_std = h[5], std_off = h[6], ragged = h[7],
            rows = h[8];
  BAD(B >= 1 && B <= 64 && T >= 1 && T <= 4096 && C >= 1 && C <= 4096 && ldx >= C && ldx <= 8192, "frame_stats: shape");
  BAD((with_std == 0 || with_std == 1) && std_off >= 0 && ldo >= (with_std ? std_off + C : C) && ldo <= 16384 &&
          (!with_std || std_off >= C),
      "frame_stats: the output row does not hold mean and std");
  BAD(rows >= 1 && rows < kMaxRows && (ragged || rows == B * T), "frame_stats: rows");
  const auto x = c.f32((long long)rows * ldx, "x");
  const auto seg = offsets(c, ragged, B, rows);
  Pool& pool = c.pool;
  const size_t n = (size_t)(B + 2) * ldo;
  float* out = pool.filled(n);
  c.result(out, n);
  c.guarded([&] {
    launch_frame_stats(pool.up(x), ldx, B, T, C, out + ldo, ldo, with_std, std_off, c.stream,
                       ragged ? pool.up(seg) : nullptr);
  });
}

void run_small_linear(Case& c) {
  const int* h = c.h;
  const int R = h[0], K = h[1], N = h[2], ldin = h[3], ldo = h[4], act = h[5], has_bias = h[6], scratch = h[7];
  BAD(R >= 1 && R <= 256 && K >= 1 && K <= 32768 && N >= 1 && N <= 4096 && ldin >= K && ldin <= 40000 && ldo >= N &&
          ldo <= 8192,
      "small_linear: shape");
  BAD(act >= 0 && act <= 3 && (has_bias == 0 || has_bias == 1) && scratch >= 0 && scratch <= 2, "small_linear: flags");
  const auto in = c.f32((long long)R * ldin, "in"), wt = c.f32((long long)K * N, "wt");
  const auto bias = c.f32(has_bias ? N : 0, "bias");
  Pool& pool = c.pool;
  const size_t n = (size_t)(R + 2) * ldo;
  float* out = pool.filled(n);
  c.result(out, n);
  c.guarded([&] {
    SmallLinearArgs a{pool.up(in), ldin, pool.up(wt), has_bias ? pool.up(bias) : nullptr, out + ldo, ldo, R, K, N, act};
    if (scratch) {
      const size_t need = small_linear_scratch_floats(R, N, K);
      BAD(need >= 1, "small_linear: this K takes no scratch");
      a.scratch = pool.filled(need);  // the whole of it, also where one float fewer is offered
      a.scratch_floats = scratch == 1 ? need : need - 1;
    }
    launch_small_linear(a, c.stream);
  });
}

void run_residual_scale(Case& c) {
  const int* h = c.h;
  const int B = h[0], T = h[1], C = h[2], has_x = h[3], ragged = h[4], M = h[5];
  BAD(B >= 1 && B <= 4096 && T >= 1 && C >= 1 && C <= 4096 && (has_x == 0 || has_x == 1), "residual_scale: shape");
  BAD(M >= 1 && M < kMaxRows && (ragged || M == (long long)B * T), "residual_scale: rows");
  const auto x = c.f32(has_x ? (long long)M * C : 0, "x"), hh = c.f32((long long)M * C, "h");
  const auto g = c.f32((long long)B * C, "g");
  const auto seg = offsets(c, ragged, B, M);
  Pool& pool = c.pool;
  const size_t n = (size_t)(M + 2) * C;
  float* out = pool.filled(n);
  c.result(out, n);
  c.guarded([&] {
    launch_residual_scale(has_x ? pool.up(x) : nullptr, pool.up(hh), pool.up(g), out + C, B, T, C, c.stream,
                          ragged ? pool.up(seg) : nullptr, M);
  });
}

void run_gate_seam(Case& c) {
  const bool seam = c.op == 8;
  const int* h = c.h;
  const int variant = h[0], B = h[1], T = h[2], N = h[3], K = h[4], gate_k0 = h[5], lda = h[6], ldg = h[7], ldo = h[8],
            ragged = h[9], M = h[10], ldh = h[11], ldso = h[12];
  BAD(variant >= 3 && variant <= 7 && B >= 1 && B <= 64 && T >= 1 && T <= 4096 && M >= 1 && M < kMaxRows &&
          (ragged || M == B * T),
      "gemm: batch");
  BAD(N >= 32 && N <= 4096 && N % 32 == 0 && K >= 64 && K <= 4096 && K % 64 == 0 && gate_k0 >= 0 && gate_k0 < K,
      "gemm: N / K / gate_k0");
  BAD(lda >= K && lda <= 8192 && ldg >= K - gate_k0 && ldg <= 8192 && ldo >= N && ldo <= 8192, "gemm: leading dimensions");
  if (seam) BAD(gate_k0 == 0 && ldh >= K && ldh <= 8192 && ldso >= K && ldso <= 8192, "seam: leading dimensions");
  const auto a = c.f32((long long)M * lda, "a"), w = c.f32((long long)N * K, "w");
  const auto bias = c.f32(N, "bias"), scale = c.f32(N, "scale"), shift = c.f32(N, "shift");
  const auto gate = c.f32((long long)B * ldg, "gate");
  const auto seg = offsets(c, ragged, B, M);
  std::vector<float> hh;
  if (seam) hh = c.f32((long long)M * ldh, "h");
  Pool& pool = c.pool;
  const size_t n = (size_t)(M + 8) * ldo, ns = seam ? (size_t)(M + 8) * ldso : 0;
  float* out = pool.filled(n);
  float* sout = seam ? pool.filled(ns) : nullptr;
  c.result(out, n);
  if (seam) c.result(sout, ns);
  c.guarded([&] {
    std::vector<uint16_t> whi, wlo;
    pack::split(pack::conv_kmajor(w, N, K, 1, K), whi, wlo);
    ConvGemmArgs p{};
    p.a[0] = p.a[1] = p.a[2] = pool.up(a);
    p.lda[0] = p.lda[1] = p.lda[2] = lda;
    p.cseg[1] = p.cseg[2] = p.cseg[3] = K;
    p.cin = K, p.taps = 1, p.dil = 1, p.pad = 0, p.M = M, p.T = T, p.N = N, p.K = p.Kp = K;
    p.bias = pool.up(bias), p.scale = pool.up(scale), p.shift = pool.up(shift);
    p.out = out + 4 * (size_t)ldo, p.ldo = ldo, p.act = kActRelu, p.amode = kACat;
    if (ragged) p.seg = pool.up(seg), p.nseg = B;
    p.gate = pool.up(gate), p.ldg = ldg, p.gate_k0 = gate_k0;
    if (seam) {
      p.role = 1;
      p.seam_h = pool.up(hh), p.ld_seam_h = ldh;
      p.seam_out = sout + 4 * (size_t)ldso, p.ld_seam_out = ldso;
    }
    c.own[0] = seam ? conv_gemm_x3_seam_ok(p, variant) : conv_gemm_x3_gate_ok(p, variant);
    launch_conv_gemm_x3(p, pool.up(whi), pool.up(wlo), variant, c.stream);
  });
}

void run_case(Case& c) {
  switch (c.op) {
    case 1: run_res2(c); break;
    case 2: run_astp_fused(c); break;
    case 3: run_astp_pool(c); break;
    case 4: run_frame_stats(c); break;
    case 5: run_small_linear(c); break;
    case 6: run_residual_scale(c); break;
    case 7:
    case 8: run_gate_seam(c); break;
    default: BAD(false, "unknown operator");
  }
}

}  // namespace

int main(int argc, char** argv) { return op_runner_main(argc, argv, "ecapa_run", 0x41505357u, Layout{16, 2, 0}, run_case); }
