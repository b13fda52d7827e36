// Tile family 7 pieces shared by its translation units (conv_gemm_x3_t6.hip: the LDS-DMA kernels;
// conv_gemm_x3_t7.hip: the seam kernel): the DMA helper, the A slot map, the LayerNorm fold helpers
// and the row-piece epilogue through LDS.
#pragma once

#include "conv_gemm_x3_impl.h"

namespace wsp {
namespace {

typedef __attribute__((address_space(3))) void lds_void;
constexpr int kGA = 256 * 128, kGW = 256 * 64, kGStage = kGA + 2 * kGW;

__device__ __forceinline__ int g_aslot(int r, int c) { return r * 128 + ((c ^ ((r >> 1) & 5)) << 4); }

__device__ __forceinline__ void g_dma(__amdgpu_buffer_rsrc_t r, unsigned char* lds, int voff) {
  __builtin_amdgcn_raw_ptr_buffer_load_lds(r, (lds_void*)lds, 16, voff, 0, 0, 0);
}

// A modes (AM): 1 = dense, 1x1 row-local GEMMs (taps 1, no padding, stride 1: A row = output row,
// also in ragged batches) keep one register per A row; 0 = convs on uniform k-tiles (one tap and
// one concat segment per k-tile) keep ALoader's (row, frame, length) triple; 2 = k-tiles that
// straddle taps (cin % 32 != 0: ECAPA layer1, cin 80) decode tap and channel per lane and 16-B
// chunk (ALoader's non-uniform path; one A segment, zeros past K).
// Epilogue through LDS: each wave parks its raw 64 x 128 accumulators, 32 rows at a time, in a
// private [32][132] fp32 block (padded rows: the 16 column lanes x rows 4q + r of a
// ds_write_b32 hit distinct banks), then walks them back row-major — lane l owns columns
// 4 (l & 31) .. + 3 and rows 2u + (l >> 5) — so every epilogue operand (bias / BN / row bias /
// residual) is one 16-B load and every output leaves in a 16-B store that, with its 31
// neighbours, writes a whole 512-B row piece (4 full 128-B lines per row instead of 64-B pieces
// of 4 rows per dword store).  Same per-element arithmetic and order as gemm_epilogue_store16.
constexpr int kGEpiLd = 132;
constexpr int kGEpiBytes = 8 * 32 * kGEpiLd * 4;
typedef unsigned u32x4 __attribute__((ext_vector_type(4)));

// LayerNorm fold (ConvGemmArgs::lnmode): mean and 1 / sqrt(var + eps) of row `row` from its
// ln_parts (mean, M2) partials of 128 columns, combined in order (Chan et al.'s pairwise update;
// every consumer of the row computes the same values).
// Each lane computes one row (the wave's 64 rows); the epilogue fetches them by lane shuffle.
constexpr int kLnMaxParts = 8;
__device__ __forceinline__ void g_ln_row(const ConvGemmArgs& p, int row, float& mu, float& rstd) {
  const float* s = p.ln_in + (size_t)row * p.ln_parts * 2;
  float m = s[0], m2 = s[1];
#pragma unroll
  for (int k = 1; k < kLnMaxParts; ++k) {
    if (k < p.ln_parts) {  // merge part k (128 values) into the first k parts (128 k values)
      const float d = s[2 * k] - m;
      m += d * (1.f / (float)(k + 1));
      m2 += s[2 * k + 1] + d * d * (128.f * (float)k / (float)(k + 1));
    }
  }
  mu = m;
  rstd = 1.f / sqrtf(m2 / (128.f * (float)p.ln_parts) + p.ln_eps);
}

// (mean, M2) of the 128 values the 32 lanes of a half-wave hold (4 each) for R rows at once ->
// lane 16 of the half (lanes 16 / 48): pairwise merges of equal counts, symmetric in the two
// partners up to the last step (same result on both); the R rows' merge chains interleave
template <int R>
__device__ __forceinline__ void g_ln_pieces(float (&m)[R], float (&m2)[R]) {
  float n = 4.f;
  auto merge = [&](int i, float mo, float m2o) {
    const float d = mo - m[i];
    m[i] = 0.5f * (m[i] + mo);
    m2[i] = (m2[i] + m2o) + d * d * (0.5f * n);
  };
#define WSP_DPP(v, ctrl) __builtin_bit_cast(float, __builtin_amdgcn_mov_dpp(__builtin_bit_cast(int, v), ctrl, 0xF, 0xF, false))
  // the first four steps inside rows of 16 lanes: quad xor 1, xor 2, then half-row / row mirrors
  // (partners already hold equal values, so a mirror is the xor 4 / 8 exchange); then xor 16
#pragma unroll
  for (int i = 0; i < R; ++i) merge(i, WSP_DPP(m[i], 0xB1), WSP_DPP(m2[i], 0xB1));
  n *= 2.f;
#pragma unroll
  for (int i = 0; i < R; ++i) merge(i, WSP_DPP(m[i], 0x4E), WSP_DPP(m2[i], 0x4E));
  n *= 2.f;
#pragma unroll
  for (int i = 0; i < R; ++i) merge(i, WSP_DPP(m[i], 0x141), WSP_DPP(m2[i], 0x141));
  n *= 2.f;
#pragma unroll
  for (int i = 0; i < R; ++i) merge(i, WSP_DPP(m[i], 0x140), WSP_DPP(m2[i], 0x140));
  n *= 2.f;
#undef WSP_DPP
  // rows 1 / 3 of 16 lanes take row 0's / 2's value (row_bcast:15): lanes 16 and 48 end with the
  // half-wave's statistics (the other rows keep their own)
#define WSP_BC15(v) \
  __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x142, 0xA, 0xF, false))
#pragma unroll
  for (int i = 0; i < R; ++i) merge(i, WSP_BC15(m[i]), WSP_BC15(m2[i]));
#undef WSP_BC15
}

template <int ACT, bool RB, bool RES, int LNM = 0>
__device__ __forceinline__ void g_epilogue_rows(const ConvGemmArgs& p, f32x4 (&acc)[4][8], int m0, int n0, int wm,
                                                int wn, int wave, int lane, unsigned char* smem, float lmu = 0.f,
                                                float lrs = 1.f) {
  float* stg = reinterpret_cast<float*>(smem) + wave * 32 * kGEpiLd;
  const int c16 = lane & 15, q = lane >> 4;
  const int cl = 4 * (lane & 31);  // this lane's 4 columns within the wave's 128
  const int col = n0 + wn * 128 + cl;
  const f32x4 bv = p.bias ? *reinterpret_cast<const f32x4*>(p.bias + col) : f32x4{0.f, 0.f, 0.f, 0.f};
  const f32x4 sc = p.scale ? *reinterpret_cast<const f32x4*>(p.scale + col) : f32x4{1.f, 1.f, 1.f, 1.f};
  const f32x4 sh = p.scale ? *reinterpret_cast<const f32x4*>(p.shift + col) : f32x4{0.f, 0.f, 0.f, 0.f};
  f32x4 lcs{0.f, 0.f, 0.f, 0.f}, lg{1.f, 1.f, 1.f, 1.f}, lb{0.f, 0.f, 0.f, 0.f};
  if constexpr ((LNM & 2) != 0) lcs = *reinterpret_cast<const f32x4*>(p.ln_cs + col);
  if constexpr ((LNM & 4) != 0) {
    lg = *reinterpret_cast<const f32x4*>(p.ln_g + col);
    lb = *reinterpret_cast<const f32x4*>(p.ln_b + col);
  }
  const int lparts = p.N / 128, lpart = (n0 + wn * 128) / 128;  // lmu / lrs: row m0 + wm * 64 + lane
  const __amdgpu_buffer_rsrc_t ro = make_rsrc(p.out);
  const __amdgpu_buffer_rsrc_t rres = make_rsrc(RES ? p.res : p.out);
#pragma unroll
  for (int h = 0; h < 2; ++h) {
    float pm[(LNM & 1) ? 16 : 1], pm2[(LNM & 1) ? 16 : 1];  // LayerNorm pieces of the half's 16 rows
#pragma unroll
    for (int i2 = 0; i2 < 2; ++i2)
#pragma unroll
      for (int j = 0; j < 8; ++j)
#pragma unroll
        for (int r = 0; r < 4; ++r) stg[(i2 * 16 + 4 * q + r) * kGEpiLd + j * 16 + c16] = acc[2 * h + i2][j][r];
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");  // wave-private block: in-order LDS, no barrier
#pragma unroll
    for (int u = 0; u < 16; ++u) {
      const int rl = 2 * u + (lane >> 5);
      const int row = m0 + wm * 64 + h * 32 + rl;
      const bool ok = row < p.M;
      const f32x4 x = *reinterpret_cast<const f32x4*>(stg + rl * kGEpiLd + cl);
      f32x4 rv{0.f, 0.f, 0.f, 0.f}, rb{0.f, 0.f, 0.f, 0.f};
      if constexpr (RES) rv = bload4(rres, ok ? (row * p.ldres + col) * 4 : kOOB);
      if constexpr (RB) {
        const int rowc = ok ? row : p.M - 1;
        const int ub = p.seg ? seg_of(p.seg, p.nseg, rowc) : rowc / p.T;
        rb = *reinterpret_cast<const f32x4*>(p.row_bias + (size_t)ub * p.N + col);
      }
      float mu = 0.f, rstd = 1.f;
      if constexpr ((LNM & 6) != 0) {  // row rl of this half: lane h * 32 + rl holds its statistics
        auto rd = [](float v, int l) {
          return __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, v), l));
        };
        mu = lane < 32 ? rd(lmu, h * 32 + 2 * u) : rd(lmu, h * 32 + 2 * u + 1);
        rstd = lane < 32 ? rd(lrs, h * 32 + 2 * u) : rd(lrs, h * 32 + 2 * u + 1);
      }
      f32x4 y;
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        float v;
        if constexpr ((LNM & 2) != 0) v = (x[e] - mu * lcs[e]) * rstd + bv[e];
        else v = x[e] + bv[e];
        if constexpr ((LNM & 4) != 0) v += (rv[e] - mu) * rstd * lg[e] + lb[e];
        else if constexpr (RES) v += rv[e];
        if constexpr (RB) v += rb[e];
        if constexpr (ACT == kActRelu) v = fmaxf(v, 0.f);
        else if constexpr (ACT == kActTanh) v = tanhf(v);
        else if constexpr (ACT == kActGelu) v = gelu_as(v);
        y[e] = v * sc[e] + sh[e];
      }
      __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4, y), ro, ok ? (row * p.ldo + col) * 4 : kOOB, 0,
                                             0);
      if constexpr ((LNM & 1) != 0) {  // this lane's 4 values of the row: (mean, M2)
        pm[u] = ((y[0] + y[1]) + (y[2] + y[3])) * 0.25f;
        float q2 = 0.f;
#pragma unroll
        for (int e = 0; e < 4; ++e) q2 += (y[e] - pm[u]) * (y[e] - pm[u]);
        pm2[u] = q2;
      }
    }
    if constexpr ((LNM & 1) != 0) {  // merge the half-wave's 32 lanes per row; lanes 16 / 48 store
      g_ln_pieces<16>(pm, pm2);
      if ((lane & 31) == 16) {
#pragma unroll
        for (int u = 0; u < 16; ++u) {
          const int row = m0 + wm * 64 + h * 32 + 2 * u + (lane >> 5);
          if (row < p.M) *reinterpret_cast<float2*>(p.ln_out + ((size_t)row * lparts + lpart) * 2) = float2{pm[u], pm2[u]};
        }
      }
    }
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");  // reads done before the next half overwrites
  }
}

}  // namespace
}  // namespace wsp
