// conv_gemm_x3 tile family 7: the 256 x 256 bf16x3 tile on 16x16x32 MFMAs with EVERY operand
// staged by LDS-DMA (buffer_load ... lds, 16 B per lane) and the fp32 A split into bf16 hi / lo
// when its fragments are read (r4; x3_variant 7).
//
// Family 6 (conv_gemm_x3<..., MF = 16>) stages A through one register set: fp32 loads, the
// hi / lo split and ds_write passes sit between the MFMA sub-steps of every k-tile, and its
// 128 accumulators leave no room for a second set (the staging costs ~20 % of
// the loop).  Here nothing passes through registers on the way to LDS: per k-tile and lane,
// four 16-B DMAs of A rows (fp32, 128-B LDS rows) and four of W (bf16 hi / lo images, 64-B
// rows) land in the free half of a two-stage ring while the other half multiplies; a k-tile
// ends with one vmcnt(0) + barrier and the next DMAs are issued right behind it.  The split
// moves to the fragment reads (8 floats -> bf16x8 hi + lo per 16x16x32 A fragment), where its
// VALU issues beside the MFMAs.  Same products, same MFMA order, same per-element epilogue
// arithmetic as family 6: bit-identical results.  The epilogue (the 256 KB C tile leaving one
// block per CU with nothing overlapping it, ~15-25 % of a block at K <= 1024) goes through LDS
// and leaves as whole 512-B row pieces in 16-B stores (g_epilogue_rows; the SE column sums
// re-read the staged outputs in family 6's summation order — bit-identical f64 partials — in
// two column passes of 64 (g_epilogue_cs, a kernel instance of its own) so that no sum stays
// live across passes).  C x C conv: bias + ReLU + BN 0.69-0.70 -> 0.64-0.65 ms, + SE column
// sums 0.78-0.80 -> 0.71-0.73 (tools/g7_check); C2 +5.2 %, C4 +3.2-3.6 % against family 6.  A transposed
// accumulator map storing 16 B per lane straight from registers (16 rows x 64 B per store) was
// slower in the model, and a persistent form fetching the next tile's first k-tiles behind the
// epilogue measured no faster (profiles/r4e_gemm_family7_experiments.txt).  r5: a ping-pong k-loop
// (the SIMD partners one barrier apart; READ / MFMA segments; 2- and 4-phase forms, the split in the
// READ segment or in the wave's own MFMA shadows) was bit-identical and never faster — the fp32 A
// split's VALU is the loop's largest overhead wherever it is placed
// (profiles/r5a_gemm_pp_experiments.txt, r5a_gemm_check.txt).
//
// LDS per stage (64 KB; two stages = 128 KB, one block of 8 waves per CU):
//   A [256 rows][32 k] fp32, 16-B chunk c of row r at slot c ^ ((r >> 1) & 5) — the two
//     ds_read_b128 of a 16x16x32 fragment (rows lane & 15, chunks 2 (lane >> 4) + {0, 1}) hit
//     16 distinct 16-B slots in every lane group (found by exhaustive search over r mod 16);
//   W hi, W lo [256 columns][32 k] bf16, family 6's {0, 2, 3, 1} row swizzle.
// A DMA lane writes LDS base + 16 lane (lane-linear), so the swizzle is applied to the SOURCE
// chunk it fetches (cdna_hip_programming.md §5.4 rule 21).
// Supported operands: 1-D convs with one or three concatenated A segments on 32-aligned k-tiles,
// or one segment on k-tiles straddling taps (taps / dilation / padding / stride / ragged batches
// as ALoader), no added operand, no grouped columns, N % 256 == 0, 16-B aligned epilogue operands —
// launch_conv_gemm_x3 routes everything else to family 6.
#include "conv_gemm_x3_g.h"

namespace wsp {
namespace {

// The SE-column-sum epilogue (CSK instances) in two column passes of 64: each wave stages its
// 64 rows x 64 columns ([64][68] fp32), writes them out row-major (16 lanes x 16 B = 256 B per
// row piece) and re-reads the staged outputs for the column sums of those 4 column tiles, so
// no column sum stays live across passes (the one-pass form spilled ~130 registers).  Sums in
// family 6's order: per lane rows 16 i + 4 q + r (i, then r), lanes l ^ 16, l ^ 32, then waves.
constexpr int kGCsLd = 68;
constexpr int kGCsBytes = 8 * 64 * kGCsLd * 4;
template <int ACT>
__device__ __forceinline__ void g_epilogue_cs(const ConvGemmArgs& p, f32x4 (&acc)[4][8], int m0, int n0, int wm,
                                              int wn, int wave, int lane, unsigned char* smem) {
  float* stg = reinterpret_cast<float*>(smem) + wave * 64 * kGCsLd;
  const int c16 = lane & 15, q = lane >> 4;
  const int cl = 4 * c16;  // this lane's 4 columns within the pass's 64
  const __amdgpu_buffer_rsrc_t ro = make_rsrc(p.out);
  // rows of this lane's sums relative to the block: side 0 below nb, side 1 from nb to mb
  const int nb = min((m0 / p.T + 1) * p.T, p.M) - m0, mb = p.M - m0;
  unsigned side0 = 0, side1 = 0;  // bit 4 i + r
#pragma unroll
  for (int k = 0; k < 16; ++k) {
    const int rr = wm * 64 + (k >> 2) * 16 + 4 * q + (k & 3);
    side0 |= (rr < nb ? 1u : 0u) << k;
    side1 |= (rr >= nb && rr < mb ? 1u : 0u) << k;
  }
  double rs[8][2];
#pragma unroll
  for (int pp = 0; pp < 2; ++pp) {
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int jj = 0; jj < 4; ++jj)
#pragma unroll
        for (int r = 0; r < 4; ++r) stg[(16 * i + 4 * q + r) * kGCsLd + 16 * jj + c16] = acc[i][4 * pp + jj][r];
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");  // wave-private block: in-order LDS, no barrier
    const int col = n0 + wn * 128 + 64 * pp + cl;
    const f32x4 bv = p.bias ? *reinterpret_cast<const f32x4*>(p.bias + col) : f32x4{0.f, 0.f, 0.f, 0.f};
    const f32x4 sc = p.scale ? *reinterpret_cast<const f32x4*>(p.scale + col) : f32x4{1.f, 1.f, 1.f, 1.f};
    const f32x4 sh = p.scale ? *reinterpret_cast<const f32x4*>(p.shift + col) : f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int u = 0; u < 16; ++u) {
      const int rl = 4 * u + q;
      const int row = m0 + wm * 64 + rl;
      float* sp = stg + rl * kGCsLd + cl;
      const f32x4 x = *reinterpret_cast<const f32x4*>(sp);
      f32x4 y;
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        float v = x[e] + bv[e];
        if constexpr (ACT == kActRelu) v = fmaxf(v, 0.f);
        else if constexpr (ACT == kActTanh) v = tanhf(v);
        else if constexpr (ACT == kActGelu) v = gelu_as(v);
        y[e] = v * sc[e] + sh[e];
      }
      __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4, y), ro,
                                             row < p.M ? (row * p.ldo + col) * 4 : kOOB, 0, 0);
      *reinterpret_cast<f32x4*>(sp) = y;
    }
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
#pragma unroll
    for (int jj = 0; jj < 4; ++jj) {
      double c0 = 0.0, c1 = 0.0;
#pragma unroll
      for (int k = 0; k < 16; ++k) {
        const double yd = (double)stg[((k >> 2) * 16 + 4 * q + (k & 3)) * kGCsLd + 16 * jj + c16];
        c0 += (side0 >> k) & 1 ? yd : 0.0;
        c1 += (side1 >> k) & 1 ? yd : 0.0;
      }
      double v0 = c0 + __shfl_xor(c0, 16);
      v0 += __shfl_xor(v0, 32);
      double v1 = c1 + __shfl_xor(c1, 16);
      v1 += __shfl_xor(v1, 32);
      rs[4 * pp + jj][0] = v0;
      rs[4 * pp + jj][1] = v1;
      __builtin_amdgcn_sched_barrier(0);  // one column tile's 16 reads at a time
    }
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");  // reads done before the next pass overwrites
  }
  __syncthreads();  // the reduction buffer overlaps other waves' staging blocks
  constexpr int BN = 256;
  double* red = reinterpret_cast<double*>(smem);  // [4 wm][2][BN], as gemm_colsum_reduce16
  if (lane < 16) {
#pragma unroll
    for (int j = 0; j < 8; ++j)
#pragma unroll
      for (int u = 0; u < 2; ++u) red[(wm * 2 + u) * BN + (wn * 8 + j) * 16 + lane] = rs[j][u];
  }
  __syncthreads();
  const int tid = threadIdx.x;
  if (tid < 2 * BN) {
    const int u = tid / BN, c = tid - u * BN;
    double v = 0.0;
#pragma unroll
    for (int w = 0; w < 4; ++w) v += red[(w * 2 + u) * BN + c];
    p.colsum[((size_t)(m0 / 256) * 2 + u) * p.N + n0 + c] = v;
  }
}

template <int AM, bool CSK, int LNM = 0>
__global__ __launch_bounds__(512, 1) void conv_gemm_g(const ConvGemmArgs p, const __bf16* __restrict__ whi,
                                                      const __bf16* __restrict__ wlo) {
  using L = Lds<true, 16>;
  // AM 3: AM 1 whose A segment 1 is the projection shortcut's 2-D strided input (ConvGemmArgs::sc2d)
  // AM 4: AM 1 whose A is multiplied by a per-utterance gate from k = gate_k0 on (ConvGemmArgs::gate):
  // the gate rows of the block's two utterances sit in LDS behind the two stages, the k-loop runs
  // as an ungated loop followed by a gated one, and a gated tile's rdA multiplies its fp32 values
  // by the row's utterance's gate chunk before the split (h * g rounded to fp32, as
  // residual_scale_kernel<false> stored it: same split, same MFMA order, bit-identical results)
  constexpr bool DENSE = AM == 1 || AM == 3 || AM == 4;
  constexpr bool GATE = AM == 4;
  static_assert(!GATE || (!CSK && LNM == 0), "the gated instance: plain epilogues only");
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = tid >> 6;
  const int ntiles = p.N / 256;
  const int mtiles = (p.M + 255) / 256;
  const int wg = xcd_remap(blockIdx.x, ntiles * mtiles);
  const int mt = wg / ntiles;
  const int nt = wg - mt * ntiles;
  const int m0 = mt * 256;
  const int n0 = nt * 256;

  // ---- A rows of this lane: DMA i (0..3) of wave w fills LDS rows (4 w + i) * 8 .. + 7, lane
  // l row + (l >> 3), slot l & 7 <- source chunk (l & 7) ^ swizzle(row) (ALoader's row logic)
  // row = 32 w + 8 i + (l >> 3): swizzle(row) = (row >> 1) & 5 = ((l >> 4) & 1) | ((i & 1) << 2)
  const int ac0 = 4 * ((lane & 7) ^ ((lane >> 4) & 1)), ac1 = ac0 ^ 16;
  int a_r[4], a_t[DENSE ? 1 : 4], a_l[DENSE ? 1 : 4], a_s[AM == 3 ? 4 : 1];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int m = m0 + (4 * wave + i) * 8 + (lane >> 3);
    if constexpr (DENSE) {
      a_r[i] = m < p.M ? m : -1;
      if constexpr (AM == 3) {  // shortcut input row of output (b, fo, to)
        const int fto = p.Fo * p.To;
        const int b = m / fto, fo = (m - b * fto) / p.To, to = m - b * fto - fo * p.To;
        a_s[i] = m < p.M ? (b * p.Fi + fo * p.stride) * p.Ti + to * p.stride : -1;
      }
    } else if (p.seg) {
      const int mm = m < p.M ? m : p.M - 1;
      const int b = seg_of(p.seg, p.nseg, mm);
      const int t = (mm - p.seg[b]) * p.stride;
      const int* is = p.iseg ? p.iseg : p.seg;
      a_r[i] = is[b] + t;
      a_t[i] = (m < p.M) ? t : -0x40000000;
      a_l[i] = is[b + 1] - is[b];
    } else {
      const int b = m / p.T;
      const int t = (m - b * p.T) * p.stride;
      a_r[i] = b * p.Ti + t;
      a_t[i] = (m < p.M) ? t : -0x40000000;  // rows >= M fail the t-range test
      a_l[i] = p.Ti;
    }
  }
  // ---- W: DMA i (0..1) of wave w fills columns (2 w + i) * 16 .. + 15 of the hi and lo images
  int woff[2];
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    const int row = (2 * wave + i) * 16 + (lane >> 2);
    const int c = (lane & 3) ^ ((0x1320 >> (4 * ((row >> 2) & 3))) & 3);
    woff[i] = ((n0 + row) * p.Kp + 8 * c) * 2;
  }
  const __amdgpu_buffer_rsrc_t rwh = make_rsrc(whi);
  const __amdgpu_buffer_rsrc_t rwl = make_rsrc(wlo);
  const int nk = p.Kp / BK;  // >= 2 (Kp % 64 == 0)
  int jt = 0, ct = 0;  // tap and channel of the next k-tile to fetch (k-tiles are fetched in order)
  auto dma = [&](int kt, int buf) {
    unsigned char* st = smem + buf * kGStage;
    const int off = jt * p.dil - p.pad;
    const float* base = p.a[0];
    int ld = p.lda[0], cl = ct;
    if (ct >= p.cseg[2]) {
      base = p.a[2];
      ld = p.lda[2];
      cl = ct - p.cseg[2];
    } else if (ct >= p.cseg[1]) {
      base = p.a[1];
      ld = p.lda[1];
      cl = ct - p.cseg[1];
    }
    const __amdgpu_buffer_rsrc_t ra = make_rsrc(base);
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      if constexpr (DENSE) {
        const int ar = AM == 3 && ct >= p.cseg[1] ? a_s[i] : a_r[i];
        g_dma(ra, st + (4 * wave + i) * 1024, ar >= 0 ? (ar * ld + cl + (i & 1 ? ac1 : ac0)) * 4 : kOOB);
      } else if constexpr (AM == 2) {
        const int k = kt * BK + (i & 1 ? ac1 : ac0);
        const int tap = k / p.cin;
        const int offk = tap * p.dil - p.pad;
        const int tt = a_t[i] + offk;
        const bool ok = k < p.K && tt >= 0 && tt < a_l[i];
        g_dma(ra, st + (4 * wave + i) * 1024, ok ? ((a_r[i] + offk) * ld + k - tap * p.cin) * 4 : kOOB);
      } else {
        const int tt = a_t[i] + off;
        const bool ok = tt >= 0 && tt < a_l[i];
        g_dma(ra, st + (4 * wave + i) * 1024, ok ? ((a_r[i] + off) * ld + cl + (i & 1 ? ac1 : ac0)) * 4 : kOOB);
      }
    }
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const int o = woff[i] + kt * 64;
      g_dma(rwh, st + kGA + (2 * wave + i) * 1024, o);
      g_dma(rwl, st + kGA + kGW + (2 * wave + i) * 1024, o);
    }
    ct += 32;
    if (ct >= p.cin) {
      ct -= p.cin;
      ++jt;
    }
  };

  const int wm = wave >> 1, wn = wave & 1;  // 4 x 2 waves of 64 x 128
  const int r16 = lane & 15, qk = lane >> 4;
  f32x4 acc[4][8];
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 8; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
  bf16x8 ah[2], al[2], bh[4], bl[4];
  // gated tiles (AM 4): gp = this lane's 8 gate values of the tile in utterance slot 0 (the
  // utterance of the block's first row); rows from g_nb on belong to slot 1, g_slot bytes further
  // (the gate tail rounded up to whole 1-KB DMA pieces: a tail of 128 or 384 columns ends inside one)
  const int g_nb = GATE ? min((m0 / p.T + 1) * p.T, p.M) - m0 : 0;
  const int g_slot = GATE ? ((p.K - p.gate_k0) * 4 + 1023) & ~1023 : 0;
  auto rdA = [&](auto gated, const unsigned char* st, int ih, const unsigned char* gp = nullptr) {
    // fp32 rows -> bf16 hi / lo fragments (no contraction: the gated product is rounded to fp32
    // before the lo term's subtraction, as the stored g * h was)
#pragma clang fp contract(off)
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const int r = wm * 64 + (ih * 2 + i) * 16 + r16;
      f32x4 x0 = *reinterpret_cast<const f32x4*>(st + g_aslot(r, 2 * qk));
      f32x4 x1 = *reinterpret_cast<const f32x4*>(st + g_aslot(r, 2 * qk + 1));
      if constexpr (decltype(gated)::value) {
        const unsigned char* gr = gp + (r >= g_nb ? g_slot : 0);
        x0 = x0 * *reinterpret_cast<const f32x4*>(gr);
        x1 = x1 * *reinterpret_cast<const f32x4*>(gr + 16);
      }
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const __bf16 h0 = (__bf16)x0[e], h1 = (__bf16)x1[e];
        ah[i][e] = h0;
        ah[i][4 + e] = h1;
        al[i][e] = (__bf16)(x0[e] - (float)h0);
        al[i][4 + e] = (__bf16)(x1[e] - (float)h1);
      }
    }
  };
  auto rdB = [&](const unsigned char* st, int jh) {
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int o = L::off(wn * 128 + (jh * 4 + j) * 16 + r16, qk * 16);
      bh[j] = *reinterpret_cast<const bf16x8*>(st + kGA + o);
      bl[j] = *reinterpret_cast<const bf16x8*>(st + kGA + kGW + o);
    }
  };
  auto mm = [&](int ih, int jh) {
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        f32x4& c = acc[ih * 2 + i][jh * 4 + j];
        c = __builtin_amdgcn_mfma_f32_16x16x32_bf16(al[i], bh[j], c, 0, 0, 0);
        c = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ah[i], bl[j], c, 0, 0, 0);
        c = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ah[i], bh[j], c, 0, 0, 0);
      }
  };

  // LayerNorm fold: this lane's row statistics, loaded ahead of the first DMAs (their latency hides
  // behind tile 0's) and held through the k-loop (2 registers)
  float lmu = 0.f, lrs = 1.f;
  if constexpr ((LNM & 6) != 0) g_ln_row(p, min(m0 + wm * 64 + lane, p.M - 1), lmu, lrs);
  if constexpr (GATE) {
    // the gate rows of utterances m0 / T and m0 / T + 1 (zeros past the batch) -> LDS behind the
    // stages, slot u at u * g_slot: 1-KB wave pieces issued ahead of tile 0's DMAs, so the first
    // counted wait below covers them (waves with no piece only have fewer operations outstanding)
    const int ppu = g_slot >> 10, b0 = m0 / p.T;  // pieces per utterance; the last one may be partly past the tail
    const int gk = p.K - p.gate_k0;
    const __amdgpu_buffer_rsrc_t rg = make_rsrc(p.gate);
#pragma unroll
    for (int i = 0; i < 4; ++i) {  // 2 g_slot <= 32 KB: at most 4 pieces per wave
      const int q = 8 * i + wave;
      if (q >= 2 * ppu) break;
      const int u = q >= ppu ? 1 : 0;
      const int gc = (q - u * ppu) * 256 + lane * 4;  // this lane's 4 gate columns
      const bool ok = (b0 + u) * p.T < p.M && gc < gk;
      g_dma(rg, smem + 2 * kGStage + q * 1024, ok ? ((b0 + u) * p.ldg + gc) * 4 : kOOB);
    }
  }
  dma(0, 0);
  dma(1, 1);
  asm volatile("s_waitcnt vmcnt(8)" ::: "memory");  // tile 0 landed (8 DMAs per k-tile and lane)
  __builtin_amdgcn_s_barrier();
  auto ktile = [&](auto gated, int kt) {
    const int buf = kt & 1;
    const unsigned char* st = smem + buf * kGStage;
    // gated tiles: the lane's gate chunks 2 qk, 2 qk + 1 of this k-tile (slot 0)
    const unsigned char* gp =
        decltype(gated)::value ? smem + 2 * kGStage + (kt * BK - p.gate_k0 + 8 * qk) * 4 : nullptr;
    // family 6's snake over the four 2 x 4 quarters of the 64 x 128 wave tile
    rdA(gated, st, 0, gp);
    rdB(st, 0);
    mm(0, 0);
    rdB(st, 1);
    mm(0, 1);
    rdA(gated, st, 1, gp);
    mm(1, 1);
    rdB(st, 0);
    mm(1, 0);
    // tile kt + 1 (issued a k-tile ago) has landed and every wave is done reading this half
    asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
    __builtin_amdgcn_sched_barrier(0);
    if (kt + 2 < nk) dma(kt + 2, buf);
  };
  // two back-to-back loops, ungated tiles then gated ones: no per-tile branch in rdA
  const int ktg = GATE ? p.gate_k0 / BK : nk;
  for (int kt = 0; kt < ktg; ++kt) ktile(std::false_type{}, kt);
  if constexpr (GATE)
    for (int kt = ktg; kt < nk; ++kt) ktile(std::true_type{}, kt);
  // no DMA is in flight and every wave is past the last reads: the epilogue may use LDS
#define WSP_GEPI(RB, RES)                                                                                   \
  switch (p.act) {                                                                                         \
    case kActRelu: g_epilogue_rows<kActRelu, RB, RES>(p, acc, m0, n0, wm, wn, wave, lane, smem); break;    \
    case kActTanh: g_epilogue_rows<kActTanh, RB, RES>(p, acc, m0, n0, wm, wn, wave, lane, smem); break;    \
    case kActGelu: g_epilogue_rows<kActGelu, RB, RES>(p, acc, m0, n0, wm, wn, wave, lane, smem); break;    \
    default: g_epilogue_rows<kActNone, RB, RES>(p, acc, m0, n0, wm, wn, wave, lane, smem); break;          \
  }
  if constexpr (LNM != 0) {  // HuBERT LayerNorm fold instances (own kernels: the others keep their code)
    if constexpr ((LNM & 5) != 0)
      g_epilogue_rows<kActNone, false, true, LNM>(p, acc, m0, n0, wm, wn, wave, lane, smem, lmu, lrs);
    else if (p.act == kActGelu)
      g_epilogue_rows<kActGelu, false, false, LNM>(p, acc, m0, n0, wm, wn, wave, lane, smem, lmu, lrs);
    else
      g_epilogue_rows<kActNone, false, false, LNM>(p, acc, m0, n0, wm, wn, wave, lane, smem, lmu, lrs);
  } else if constexpr (CSK) {  // SE column sums: own kernel instance (its epilogue's registers stay out of the others)
    switch (p.act) {
      case kActRelu: g_epilogue_cs<kActRelu>(p, acc, m0, n0, wm, wn, wave, lane, smem); break;
      case kActTanh: g_epilogue_cs<kActTanh>(p, acc, m0, n0, wm, wn, wave, lane, smem); break;
      case kActGelu: g_epilogue_cs<kActGelu>(p, acc, m0, n0, wm, wn, wave, lane, smem); break;
      default: g_epilogue_cs<kActNone>(p, acc, m0, n0, wm, wn, wave, lane, smem); break;
    }
  } else if (p.res) {
    WSP_GEPI(false, true)
  } else if (p.row_bias) {
    WSP_GEPI(true, false)
  } else {
    WSP_GEPI(false, false)
  }
#undef WSP_GEPI
}

}  // namespace

namespace x3 {

bool g256_supported(const ConvGemmArgs& p) {
  auto a16 = [](const void* q) { return (reinterpret_cast<uintptr_t>(q) & 15) == 0; };
  const bool aligned = a16(p.out) && p.ldo % 4 == 0 && a16(p.bias) && a16(p.scale) && a16(p.shift) &&
                       a16(p.row_bias) && a16(p.res) && (!p.res || p.ldres % 4 == 0);
  // non-uniform k-tiles (AM 2): one A segment only, as ALoader's per-lane path
  return aligned && p.N % 256 == 0 && !p.conv2d && !p.gcols && p.amode == kACat &&
         (uniform_ktiles(p) || (p.cseg[1] >= p.cin && !p.colsum)) &&
         (!p.sc2d || (uniform_ktiles(p) && !p.colsum && !p.lnmode && !p.row_bias));
}

// The gated A tail (AM 4): a dense 1x1 GEMM on uniform k-tiles over a uniform batch whose
// utterances span at least a block of rows (a 256-row tile then touches at most two), no padded
// k-tiles, a gate tail of whole k-tile groups (128 columns) whose 1-KB DMA pieces per utterance fit the
// 32 KB behind the stages.
bool g256_gate_supported(const ConvGemmArgs& p) {
  if (!p.gate || !g256_supported(p) || !uniform_ktiles(p)) return false;
  const bool dense = p.taps == 1 && p.pad == 0 && p.stride == 1 && !p.iseg && !p.seg && p.Ti == p.T;
  const int gk = p.K - p.gate_k0;
  return dense && p.T >= 256 && p.M % p.T == 0 && !p.colsum && !p.lnmode && !p.sc2d && p.K == p.Kp &&
         p.gate_k0 >= 0 && p.gate_k0 % 32 == 0 && gk > 0 && gk % 128 == 0 && gk <= 4096 && p.ldg >= gk &&
         p.ldg % 4 == 0 && (reinterpret_cast<uintptr_t>(p.gate) & 15) == 0 &&
         (long long)(p.M / p.T) * p.ldg * 4 < (long long)kOOB;
}

void t_g256(const ConvGemmArgs& p, const __bf16* h, const __bf16* l, hipStream_t s) {
  const int nwg = ((p.M + 255) / 256) * (p.N / 256);
  constexpr int lds0 = 2 * kGStage > kGEpiBytes ? 2 * kGStage : kGEpiBytes;
  constexpr int lds = lds0 > kGCsBytes ? lds0 : kGCsBytes;
  // AM 1 reads A row m for output row m: only when ALoader's row map is the identity (no separate
  // input offsets, and uniform batches with Ti == T); ragged iseg / Ti != T 1x1 GEMMs take AM 0.
  const bool dense = p.taps == 1 && p.pad == 0 && p.stride == 1 && !p.iseg && (p.seg || p.Ti == p.T);
  const int am = !uniform_ktiles(p) ? 2 : dense ? 1 : 0;
  if (p.gate) {
    WSP_CHECK(g256_gate_supported(p), "conv_gemm_x3: the gated A tail needs a dense 1x1 GEMM over a uniform batch");
    // the two gate rows behind the stages, each in whole 1-KB pieces (the kernel's g_slot)
    const int ldsg = std::max(lds, 2 * kGStage + 2 * (((p.K - p.gate_k0) * 4 + 1023) & ~1023));
    hipLaunchKernelGGL((conv_gemm_g<4, false>), dim3(nwg), dim3(512), ldsg, s, p, h, l);
    WSP_HIP(hipGetLastError());
    return;
  }
  if (p.sc2d) {  // conv3 + projection shortcut (check_conv_args / g256_supported: dense, uniform k-tiles)
    hipLaunchKernelGGL((conv_gemm_g<3, false>), dim3(nwg), dim3(512), lds, s, p, h, l);
    WSP_HIP(hipGetLastError());
    return;
  }
  if (p.lnmode) {
    // LayerNorm fold: 1 = emit (out_proj / fc2 on the residual), 2 = fold (qkv / fc1), 4 = residual
    // normalised on the fly, 5 = both (fc2 / out_proj under the full fold)
    WSP_CHECK(am == 1 && !p.colsum && !p.row_bias && !p.scale && p.N % 128 == 0 &&
                  ((p.lnmode & 1) == 0 || (p.ln_out && p.res && p.act == kActNone)) &&
                  ((p.lnmode & 6) == 0 || (p.ln_in && p.ln_parts >= 1 && p.ln_parts <= kLnMaxParts)) && ((p.lnmode & 2) == 0 || (p.ln_cs && !p.res)) &&
                  (p.lnmode != 2 || p.act == kActNone || p.act == kActGelu) &&  // the fold's two epilogue instances
                  ((p.lnmode & 4) == 0 || (p.ln_g && p.ln_b && p.res && p.act == kActNone)),
              "conv_gemm_x3: LayerNorm fold needs a dense 1x1 GEMM and its operands (fold: no activation or GELU)");
    switch (p.lnmode) {
      case 1: hipLaunchKernelGGL((conv_gemm_g<1, false, 1>), dim3(nwg), dim3(512), lds, s, p, h, l); break;
      case 2: hipLaunchKernelGGL((conv_gemm_g<1, false, 2>), dim3(nwg), dim3(512), lds, s, p, h, l); break;
      case 4: hipLaunchKernelGGL((conv_gemm_g<1, false, 4>), dim3(nwg), dim3(512), lds, s, p, h, l); break;
      case 5: hipLaunchKernelGGL((conv_gemm_g<1, false, 5>), dim3(nwg), dim3(512), lds, s, p, h, l); break;
      default: WSP_CHECK(false, "conv_gemm_x3: lnmode must be 1, 2, 4 or 5");
    }
    WSP_HIP(hipGetLastError());
    return;
  }
  if (p.colsum && am == 1)
    hipLaunchKernelGGL((conv_gemm_g<1, true>), dim3(nwg), dim3(512), lds, s, p, h, l);
  else if (p.colsum && am == 0)
    hipLaunchKernelGGL((conv_gemm_g<0, true>), dim3(nwg), dim3(512), lds, s, p, h, l);
  else if (am == 1)
    hipLaunchKernelGGL((conv_gemm_g<1, false>), dim3(nwg), dim3(512), lds, s, p, h, l);
  else if (am == 0)
    hipLaunchKernelGGL((conv_gemm_g<0, false>), dim3(nwg), dim3(512), lds, s, p, h, l);
  else
    hipLaunchKernelGGL((conv_gemm_g<2, false>), dim3(nwg), dim3(512), lds, s, p, h, l);
  WSP_HIP(hipGetLastError());
}

}  // namespace x3
}  // namespace wsp
