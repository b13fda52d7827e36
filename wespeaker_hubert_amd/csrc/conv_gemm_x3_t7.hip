// conv_gemm_x3 tile family 7, the SE-Res2Block seam (x3_variant 7; ConvGemmArgs::seam_h): the next
// block's conv1 (a dense C x C GEMM) whose A operand is the previous block's output
//   v = x + g[utt] (.) h      (fma(h, g, x): what residual_scale_kernel<true> stores)
// formed while A is staged, so the residual pass — 2 reads + 1 write of [M][C] at its own HBM roof —
// disappears as a launch.  v is written once to seam_out on the way (conv_cat and the following seam
// still read x_{L+1}): the blocks of a row tile share its k-tiles out between them (block nt stores the
// k-tiles kt with kt % ntiles == nt), each row piece one whole 128-B line.
//
// Same 256 x 256 tile, 8 waves, 16x16x32 MFMAs, product order and snake as families 6 / 7, and
// family 7's row-piece epilogue: the outputs equal family 7 on the materialised tensor bit for bit.
//   W   by LDS-DMA exactly as family 7 (no staging registers), one k-tile ahead;
//   A   through one register set: tile k+1 (loaded during k-1) is combined, split ONCE per block
//       into bf16 hi / lo and written to the free stage, two of the thread's four rows in each half
//       of tile k, and the rows' registers are reloaded with tile k+2 right behind.  A 1 MFMA : 2 VALU
//       pipeline is requested for both halves; the scheduler honours it in the second (standalone
//       0.875 -> 0.809 ms at the C2 shape) and leaves the first half's staging as a block behind its
//       MFMAs (profiles/r8a_seam_fold.txt).  The fragment reads are then two ds_read_b128 with no
//       VALU split in the k-loop.
// LDS: 2 stages x (A hi, A lo, W hi, W lo: 16 KB each) = 128 KB, then the gate rows of the (at most
// two) utterances the tile touches (2 x K floats).  Preconditions as the gated tail (AM 4): uniform
// batch, T >= 256, M % T == 0.  A plain one-tile-per-block launch: no block waits for another.
//
// vmcnt bookkeeping of a k-tile, in issue order: 4 W DMAs (top), then 4 sum stores and 8 A loads.  The
// tile ends with vmcnt(12): the W DMAs, which the compiler cannot see as LDS writes, have landed.  All
// three are issued for every tile (out-of-range offsets for the tiles past the end and for the sum
// stores of the other blocks' k-tiles: loads return zeros, stores are dropped), so the stream is
// branch-free, the count holds and the compiler's own waits never reach a W DMA.
#include "conv_gemm_x3_g.h"

namespace wsp {
namespace {

constexpr int kSPlane = 256 * 64;     // one bf16 image of a 256 x 32 tile (A or W)
constexpr int kSStage = 4 * kSPlane;  // A hi, A lo, W hi, W lo

// BAL: the sum stores are shared out between the row tile's blocks; otherwise its nt == 0 block
// stores every k-tile
template <bool BAL>
__global__ __launch_bounds__(512, 1) void conv_gemm_seam(const ConvGemmArgs p, const __bf16* __restrict__ whi,
                                                         const __bf16* __restrict__ wlo) {
  using L = Lds<true, 16>;
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
  const int nk = p.K / BK;  // >= 2

  // ---- A: thread -> rows srow + 64 i (i = 0..3), floats 4 c8 .. + 3 of the k-tile; the 8 threads
  // of a row piece read and write one 128-B line
  const int srow = tid >> 3, c8 = tid & 7;
  const __amdgpu_buffer_rsrc_t rx = make_rsrc(p.a[0]);
  const __amdgpu_buffer_rsrc_t rh = make_rsrc(p.seam_h);
  const __amdgpu_buffer_rsrc_t rs = make_rsrc(p.seam_out);
  const int g_nb = min((m0 / p.T + 1) * p.T, p.M) - m0;  // rows from g_nb on: the next utterance
  int a_r[4];
  bool a_u[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int r = srow + 64 * i;
    a_r[i] = m0 + r < p.M ? m0 + r : -1;
    a_u[i] = r >= g_nb;
  }
  f32x4 vx[4], vh[4];
  auto load_a = [&](int kt, int i0) {  // rows i0, i0 + 1 of the register set
    const int kc = kt * BK + 4 * c8;
#pragma unroll
    for (int i = i0; i < i0 + 2; ++i) {
      const bool ok = kt < nk && a_r[i] >= 0;
      vx[i] = bload4(rx, ok ? (a_r[i] * p.lda[0] + kc) * 4 : kOOB);
      vh[i] = bload4(rh, ok ? (a_r[i] * p.ld_seam_h + kc) * 4 : kOOB);
    }
  };
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
  auto dma_w = [&](int kt, int buf) {
    unsigned char* st = smem + buf * kSStage;
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const int o = kt < nk ? woff[i] + kt * 64 : kOOB;
      g_dma(rwh, st + 2 * kSPlane + (2 * wave + i) * 1024, o);
      g_dma(rwl, st + 3 * kSPlane + (2 * wave + i) * 1024, o);
    }
  };
  // ---- the gate rows of utterances m0 / T and m0 / T + 1 (zeros past the batch) behind the stages
  unsigned char* const gl = smem + 2 * kSStage;
  {
    const __amdgpu_buffer_rsrc_t rg = make_rsrc(p.gate);
    const int b0 = m0 / p.T, nch = p.K / 4;
    for (int q = tid; q < 2 * nch; q += 512) {
      const int u = q >= nch ? 1 : 0;
      const bool ok = (b0 + u) * p.T < p.M;
      *reinterpret_cast<f32x4*>(gl + q * 16) = bload4(rg, ok ? ((b0 + u) * p.ldg + 4 * (q - u * nch)) * 4 : kOOB);
    }
  }

  int own = BAL ? nt : 0;  // the next k-tile whose sum this block stores
  // rows i0, i0 + 1 of tile kt in the register set: v = fma(h, g, x) (the rounding of
  // residual_scale_kernel<true>), stored as fp32 if the tile is this block's, split into bf16
  // hi / lo -> stage buf
  auto store_rows = [&](int kt, int buf, int i0) {
#pragma clang fp contract(off)
    unsigned char* st = smem + buf * kSStage;
    const int kc = kt * BK + 4 * c8;
    const int kg = kt < nk ? kc : 4 * c8;  // the past-the-end tile (zeros nobody reads) stays inside the gate rows
    const f32x4 g0 = *reinterpret_cast<const f32x4*>(gl + kg * 4);
    const f32x4 g1 = *reinterpret_cast<const f32x4*>(gl + (p.K + kg) * 4);
    const bool mine = (BAL || nt == 0) && kt == own && kt < nk;
    if (mine && i0 == 2) own += BAL ? ntiles : 1;
#pragma unroll
    for (int i = i0; i < i0 + 2; ++i) {
      const f32x4 g = a_u[i] ? g1 : g0;
      f32x4 v;
      bf16x4 hi, lo;
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        v[e] = __builtin_fmaf(vh[i][e], g[e], vx[i][e]);
        const __bf16 hh = (__bf16)v[e];
        hi[e] = hh;
        lo[e] = (__bf16)(v[e] - (float)hh);
      }
      __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4, v), rs,
                                             mine && a_r[i] >= 0 ? (a_r[i] * p.ld_seam_out + kc) * 4 : kOOB, 0, 0);
      const int off = L::off(srow + 64 * i, c8 * 8);
      *reinterpret_cast<bf16x4*>(st + off) = hi;
      *reinterpret_cast<bf16x4*>(st + kSPlane + off) = lo;
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
  auto rdA = [&](const unsigned char* st, int ih) {
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const int o = L::off(wm * 64 + (ih * 2 + i) * 16 + r16, qk * 16);
      ah[i] = *reinterpret_cast<const bf16x8*>(st + o);
      al[i] = *reinterpret_cast<const bf16x8*>(st + kSPlane + o);
    }
  };
  auto rdB = [&](const unsigned char* st, int jh) {
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int o = L::off(wn * 128 + (jh * 4 + j) * 16 + r16, qk * 16);
      bh[j] = *reinterpret_cast<const bf16x8*>(st + 2 * kSPlane + o);
      bl[j] = *reinterpret_cast<const bf16x8*>(st + 3 * kSPlane + o);
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

  // one MFMA, then two of the staging's VALU instructions, for the 48 MFMAs of half a k-tile: the
  // combine / split of two rows issues in the MFMAs' shadow instead of ahead of them
  auto interleave = [] {
#pragma unroll
    for (int z = 0; z < 48; ++z) {
      __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
      __builtin_amdgcn_sched_group_barrier(0x002, 2, 0);
    }
  };
  load_a(0, 0);
  load_a(0, 2);
  dma_w(0, 0);
  asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");  // gate rows written, W tile 0 landed
  __builtin_amdgcn_s_barrier();
  __builtin_amdgcn_sched_barrier(0);
  store_rows(0, 0, 0);
  store_rows(0, 0, 2);
  load_a(1, 0);
  load_a(1, 2);
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
  __builtin_amdgcn_s_barrier();
  __builtin_amdgcn_sched_barrier(0);
  for (int kt = 0; kt < nk; ++kt) {
    const int buf = kt & 1;
    const unsigned char* st = smem + buf * kSStage;
    dma_w(kt + 1, buf ^ 1);  // every wave is past its reads of that stage
    __builtin_amdgcn_sched_barrier(0);
    // each half of the tile: two rows of tile kt + 1 (loaded a k-tile ago) -> the free stage, their
    // registers reloaded with tile kt + 2 (out-of-range past the end: zeros nobody reads).  Written
    // after the fragment reads: LDS writes the compiler cannot tell from those reads' stage would
    // otherwise pin the whole staging ahead of the MFMAs
    rdA(st, 0);
    rdB(st, 0);
    mm(0, 0);
    rdB(st, 1);
    mm(0, 1);
    store_rows(kt + 1, buf ^ 1, 0);
    load_a(kt + 2, 0);
    interleave();
    __builtin_amdgcn_sched_barrier(0);
    rdA(st, 1);
    mm(1, 1);
    rdB(st, 0);
    mm(1, 0);
    store_rows(kt + 1, buf ^ 1, 2);
    load_a(kt + 2, 2);
    interleave();
    // W tile kt + 1 has landed (12 operations follow its DMAs: the tile's 4 sum stores and 8 A
    // loads), this wave's A pieces are written and its reads of this stage are done
    asm volatile("s_waitcnt vmcnt(12) lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
    __builtin_amdgcn_sched_barrier(0);
  }
  // only out-of-range A loads are in flight and every wave is past the last reads: the epilogue may use LDS
  switch (p.act) {
    case kActRelu: g_epilogue_rows<kActRelu, false, false>(p, acc, m0, n0, wm, wn, wave, lane, smem); break;
    case kActTanh: g_epilogue_rows<kActTanh, false, false>(p, acc, m0, n0, wm, wn, wave, lane, smem); break;
    case kActGelu: g_epilogue_rows<kActGelu, false, false>(p, acc, m0, n0, wm, wn, wave, lane, smem); break;
    default: g_epilogue_rows<kActNone, false, false>(p, acc, m0, n0, wm, wn, wave, lane, smem); break;
  }
}

}  // namespace

namespace x3 {

// The seam: a dense 1x1 GEMM with one A segment on uniform k-tiles over a uniform batch whose
// utterances span at least a block of rows (a 256-row tile then touches at most two), no padded
// k-tiles, a plain epilogue (bias, activation, scale / shift), a gate over all of K whose two rows fit
// the 32 KB behind the stages, and 16-B aligned operands below 2 GiB.
bool seam_supported(const ConvGemmArgs& p) {
  if (!p.seam_h || !p.seam_out || !p.gate || !g256_supported(p) || !uniform_ktiles(p)) return false;
  auto a16 = [](const void* q) { return (reinterpret_cast<uintptr_t>(q) & 15) == 0; };
  const bool dense = p.taps == 1 && p.pad == 0 && p.stride == 1 && !p.iseg && !p.seg && p.Ti == p.T && p.cseg[1] == p.cin;
  const bool plain = !p.colsum && !p.lnmode && !p.sc2d && !p.res && !p.row_bias;
  const bool lds = p.K == p.Kp && p.K % 64 == 0 && p.K <= 4096;
  const bool ops = a16(p.a[0]) && a16(p.seam_h) && a16(p.seam_out) && a16(p.gate) && p.gate_k0 == 0 && p.ldg >= p.K &&
                   p.ldg % 4 == 0 && p.lda[0] >= p.K && p.ld_seam_h >= p.K && p.ld_seam_h % 4 == 0 &&
                   p.ld_seam_out >= p.K && p.ld_seam_out % 4 == 0;
  if (!dense || !plain || !lds || !ops || p.T < 256 || p.M % p.T != 0) return false;
  const long long lim = kOOB;
  return (long long)(p.M / p.T) * p.ldg * 4 < lim && (long long)p.M * p.ld_seam_h * 4 < lim &&
         (long long)p.M * p.ld_seam_out * 4 < lim;
}

void t_seam(const ConvGemmArgs& p, const __bf16* h, const __bf16* l, hipStream_t s, bool balanced) {
  WSP_CHECK(seam_supported(p), "conv_gemm_x3: the seam needs a dense 1x1 GEMM over a uniform batch with T >= 256");
  const int nwg = ((p.M + 255) / 256) * (p.N / 256);
  const int lds = std::max(2 * kSStage + 2 * p.K * 4, kGEpiBytes);
  if (balanced)
    hipLaunchKernelGGL((conv_gemm_seam<true>), dim3(nwg), dim3(512), lds, s, p, h, l);
  else
    hipLaunchKernelGGL((conv_gemm_seam<false>), dim3(nwg), dim3(512), lds, s, p, h, l);
  WSP_HIP(hipGetLastError());
}

}  // namespace x3
}  // namespace wsp
