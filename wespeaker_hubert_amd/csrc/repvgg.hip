// RepVGG / RepSPK kernels (repvgg.h has the contracts).
//
// rsbb_conv_kernel is the conv-GEMM family's bf16x3 implicit GEMM (conv_gemm_x3_impl.h) with a third
// A-loader beside ALoader / ALoader2D: the tap of a k-tile walks the 17-entry live-tap table of a folded
// RepSPK 5x5 kernel instead of all kh x kw taps, so the eight structurally zero taps cost neither loads
// nor MFMAs (K = 17 cin instead of 25 cin).  Same staging (fp32 A split into bf16 hi / lo on the way to
// LDS, W pre-split, swizzled 64-byte LDS rows, two register sets, two LDS stages), the same product (bf16x3.h
// mma3) and the same epilogue (gemm_common.h gemm_epilogue).  Block = 4 waves on 128 rows, each wave
// 32 rows x TN column tiles of 32.
#include "bf16x3.h"
#include "gemm_common.h"
#include "repvgg.h"

namespace wsp {

namespace {

constexpr int BK = 32;
constexpr int ROWB = 64;  // one k-tile row: 32 bf16, unpadded
// LDS byte offset of `byte` in row `row`: the row's four 16-byte chunks XOR-swizzled by (row >> 2) & 3, which
// keeps the fragment reads (row = lane & 31, chunk = 2 s + h) conflict-free without padding
// (conv_gemm_x3_impl.h Lds<true>): two 128 x 128 blocks fit a CU
__device__ __forceinline__ int lds_off(int row, int byte) {
  return row * 64 + ((((byte >> 4) ^ (row >> 2)) & 3) << 4) + (byte & 15);
}

// the live-tap table, 3 bits per entry
constexpr unsigned long long tap_bits(int which) {
  unsigned long long v = 0;
  for (int j = 0; j < kRsbbLiveTaps; ++j) v |= (unsigned long long)kRsbbTaps[j][which] << (3 * j);
  return v;
}
constexpr unsigned long long kKfBits = tap_bits(0), kKtBits = tap_bits(1);

// Rows are output positions (b, fo, to) of an NHWC plane, as ALoader2D; the tap of the current k-tile is
// entry j of the live-tap table (cin % 32 == 0: a k-tile never straddles two taps).
template <int AR>
struct ALoaderTaps {
  const float* a0;
  int ld, cin, Fi, Ti;
  int c4;
  int rb[AR], fi0[AR], ti0[AR];
  int j, c;

  __device__ __forceinline__ void init(const ConvGemmArgs& p, int m0, int srow, int rows_step, int c4_) {
    a0 = p.a[0];
    ld = p.lda[0];
    cin = p.cin;
    Fi = p.Fi;
    Ti = p.Ti;
    c4 = c4_;
    j = 0;
    c = 0;
    const int plane = p.Fo * p.To;
#pragma unroll
    for (int i = 0; i < AR; ++i) {
      const int m = m0 + srow + rows_step * i;
      const int b = m / plane;
      const int rem = m - b * plane;
      const int fo = rem / p.To;
      const int to = rem - fo * p.To;
      rb[i] = b * p.Fi * p.Ti;
      fi0[i] = (m < p.M) ? fo * p.stride - 2 : -0x40000000;  // invalid rows fail the range test
      ti0[i] = to * p.stride - 2;
    }
  }

  // the next k-tile; `live` = false (and the zero tail of the packed K) issues out-of-range loads: zeros
  __device__ __forceinline__ void load(f32x4 (&ra)[AR], bool live) {
    const bool tap = live && j < kRsbbLiveTaps;
    const int sh = 3 * (j < kRsbbLiveTaps ? j : 0);
    const int kf = (int)((kKfBits >> sh) & 7), kt = (int)((kKtBits >> sh) & 7);
    const __amdgpu_buffer_rsrc_t r0 = make_rsrc(a0);
#pragma unroll
    for (int i = 0; i < AR; ++i) {
      const int fi = fi0[i] + kf;
      const int ti = ti0[i] + kt;
      const bool ok = tap && fi >= 0 && fi < Fi && ti >= 0 && ti < Ti;
      const int row = rb[i] + fi * Ti + ti;
      ra[i] = bload4(r0, ok ? (row * ld + c + c4) * 4 : kOOB);
    }
    c += 32;
    if (c >= cin) {
      c -= cin;
      ++j;
    }
  }
};

template <int TN>
__global__ __launch_bounds__(256, 2) void rsbb_conv_kernel(const ConvGemmArgs p, const __bf16* __restrict__ whi,
                                                           const __bf16* __restrict__ wlo) {
  constexpr int NT = 256, TM = 1;  // 4 waves on M
  constexpr int BM = 128, BN = TN * 32;
  constexpr int AR = BM * 8 / NT;  // float4 A loads per thread per k-tile
  constexpr int BR = BN * 8 / NT;  // 16-byte W loads per thread per k-tile (hi + lo)
  constexpr int ROWS_A = NT / 8;
  constexpr int A_BYTES = BM * ROWB;
  constexpr int B_BYTES = BN * ROWB;
  constexpr int B_LO = B_BYTES;
  constexpr int STAGE = 2 * A_BYTES + B_LO + B_BYTES;
  static_assert(BR >= 1 && BN * 4 % 64 == 0, "a W image must be a whole number of wave loads");

  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = tid >> 6;
  const int ntiles = p.N / BN;
  const int mtiles = (p.M + BM - 1) / BM;
  const int wg = xcd_remap(blockIdx.x, ntiles * mtiles);
  const int mt = wg / ntiles;
  const int nt = wg - mt * ntiles;
  const int m0 = mt * BM;
  const int n0 = nt * BN;

  const int srow = tid >> 3;
  const int c4 = (tid & 7) * 4;
  ALoaderTaps<AR> al;
  al.init(p, m0, srow, ROWS_A, c4);
  // W staging: 16-byte chunk q = tid + NT * i over both images (BN * 4 chunks each; the image is wave-uniform)
  const __amdgpu_buffer_rsrc_t rwhi = make_rsrc(whi);
  const __amdgpu_buffer_rsrc_t rwlo = make_rsrc(wlo);
  int boff[BR], bls[BR];
  bool bimg[BR];
#pragma unroll
  for (int i = 0; i < BR; ++i) {
    const int q = tid + NT * i;
    const int img = __builtin_amdgcn_readfirstlane(q / (BN * 4));
    const int qq = q - img * BN * 4;
    const int row = qq >> 2, part = qq & 3;
    bimg[i] = img != 0;
    boff[i] = ((n0 + row) * p.Kp + part * 8) * 2;
    bls[i] = lds_off(row, part * 16) + (img ? B_LO : 0);
  }

  f32x4 ra0[AR], ra1[AR];
  bf16x8 rb0[BR], rb1[BR];

  auto load_tile = [&](f32x4(&ra)[AR], bf16x8(&rb)[BR], int k0, bool live) {
#pragma unroll
    for (int i = 0; i < BR; ++i) {
      const int o = live ? boff[i] + k0 * 2 : kOOB;
      rb[i] = __builtin_bit_cast(bf16x8, __builtin_amdgcn_raw_buffer_load_b128(bimg[i] ? rwlo : rwhi, o, 0, 0));
    }
    al.load(ra, live);
  };

  auto store_tile = [&](const f32x4(&ra)[AR], const bf16x8(&rb)[BR], int buf) {
    unsigned char* st = smem + buf * STAGE;
#pragma unroll
    for (int i = 0; i < AR; ++i) {
      bf16x4 hi, lo;
      split(ra[i], hi, lo);
      const int off = lds_off(srow + ROWS_A * i, c4 * 2);
      *reinterpret_cast<bf16x4*>(st + off) = hi;
      *reinterpret_cast<bf16x4*>(st + A_BYTES + off) = lo;
    }
#pragma unroll
    for (int i = 0; i < BR; ++i) *reinterpret_cast<bf16x8*>(st + 2 * A_BYTES + bls[i]) = rb[i];
  };

  const int wm = wave;  // WN = 1
  const int r32 = lane & 31;
  const int h = lane >> 5;

  f32x16 acc[TM][TN];
#pragma unroll
  for (int jn = 0; jn < TN; ++jn)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[0][jn][r] = 0.f;

  auto mma_step = [&](int buf, int s) {
    const unsigned char* st = smem + buf * STAGE;
    const unsigned char* a_hi = st + lds_off(wm * 32 + r32, h * 16 + s * 32);
    const unsigned char* a_lo = a_hi + A_BYTES;
    const unsigned char* b_hi = st + 2 * A_BYTES + lds_off(r32, h * 16 + s * 32);  // rows 32 jn + r32 swizzle alike
    const unsigned char* b_lo = b_hi + B_LO;
    const bf16x8 ah = *reinterpret_cast<const bf16x8*>(a_hi);
    const bf16x8 al_ = *reinterpret_cast<const bf16x8*>(a_lo);
    bf16x8 bh[TN], bl[TN];
#pragma unroll
    for (int jn = 0; jn < TN; ++jn) {
      bh[jn] = *reinterpret_cast<const bf16x8*>(b_hi + jn * 32 * ROWB);
      bl[jn] = *reinterpret_cast<const bf16x8*>(b_lo + jn * 32 * ROWB);
    }
#pragma unroll
    for (int jn = 0; jn < TN; ++jn) mma3(ah, al_, bh[jn], bl[jn], acc[0][jn]);
  };

  // nk is even (Kp % 64 == 0, checked on the host); loads and stores are unconditional (past-the-end tiles
  // load zeros into a buffer nobody reads), as in conv_gemm_x3
  const int nk = p.Kp / BK;
  load_tile(ra0, rb0, 0, true);
  load_tile(ra1, rb1, BK, true);
  store_tile(ra0, rb0, 0);
  __syncthreads();
  for (int kt = 0; kt < nk; kt += 2) {
    load_tile(ra0, rb0, (kt + 2) * BK, kt + 2 < nk);
    mma_step(0, 0);
    store_tile(ra1, rb1, 1);
    mma_step(0, 1);
    __syncthreads();
    load_tile(ra1, rb1, (kt + 3) * BK, kt + 3 < nk);
    mma_step(1, 0);
    store_tile(ra0, rb0, 0);
    mma_step(1, 1);
    __syncthreads();
  }
  gemm_epilogue<TM, TN>(p, acc, m0, n0, wm, 0, lane);
}

template <int TN>
void launch_rsbb_k(const ConvGemmArgs& g, const void* whi, const void* wlo, hipStream_t s) {
  constexpr int BM = 128, BN = TN * 32;
  const int nwg = ((g.M + BM - 1) / BM) * (g.N / BN);
  const size_t lds = (size_t)2 * (2 * BM * ROWB + 2 * BN * ROWB);
  hipLaunchKernelGGL((rsbb_conv_kernel<TN>), dim3(nwg), dim3(256), lds, s, g, static_cast<const __bf16*>(whi),
                     static_cast<const __bf16*>(wlo));
  WSP_HIP(hipGetLastError());
}

// ------------------------------------------------------------------ stem ---
// one thread per position: its TAPS inputs in registers, the weights in LDS, C0 channels as float4 stores
template <int C0, int TAPS>
__global__ __launch_bounds__(256) void repvgg_stem_kernel(const float* __restrict__ feats, int T, int F,
                                                          const float* __restrict__ w, const float* __restrict__ bias,
                                                          float* __restrict__ out, int ldo, int Cpad, long total) {
  __shared__ float s_w[C0 * TAPS];
  __shared__ float s_b[C0];
  for (int i = threadIdx.x; i < C0 * TAPS; i += 256) s_w[i] = w[i];
  for (int i = threadIdx.x; i < C0; i += 256) s_b[i] = bias[i];
  __syncthreads();
  const long idx = blockIdx.x * 256L + threadIdx.x;
  if (idx >= total) return;
  const int t = (int)(idx % T);
  const long bf = idx / T;
  const int f = (int)(bf % F);
  const int b = (int)(bf / F);
  float x[TAPS];
#pragma unroll
  for (int q = 0; q < TAPS; ++q) {
    const int ff = f + (TAPS == 9 ? q / 3 - 1 : TAPS == 25 ? q / 5 - 2 : (int)((kKfBits >> (3 * q)) & 7) - 2);
    const int tt = t + (TAPS == 9 ? q % 3 - 1 : TAPS == 25 ? q % 5 - 2 : (int)((kKtBits >> (3 * q)) & 7) - 2);
    x[q] = (ff >= 0 && ff < F && tt >= 0 && tt < T) ? feats[((long)b * T + tt) * F + ff] : 0.f;
  }
  f32x4* o = reinterpret_cast<f32x4*>(out + idx * ldo);
#pragma unroll
  for (int q4 = 0; q4 < C0 / 4; ++q4) {
    f32x4 v;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const int ch = q4 * 4 + e;
      float a = s_b[ch];
#pragma unroll
      for (int q = 0; q < TAPS; ++q) a = fmaf(x[q], s_w[ch * TAPS + q], a);
      v[e] = fmaxf(a, 0.f);
    }
    o[q4] = v;
  }
  for (int q4 = C0 / 4; q4 < Cpad / 4; ++q4) o[q4] = f32x4{0.f, 0.f, 0.f, 0.f};
}

template <int C0>
void launch_stem_c(const RepvggStemArgs& p, long total, hipStream_t s) {
  const unsigned grid = (unsigned)((total + 255) / 256);
  if (p.taps == 9)
    hipLaunchKernelGGL((repvgg_stem_kernel<C0, 9>), dim3(grid), dim3(256), 0, s, p.feats, p.T, p.F, p.w, p.bias, p.out,
                       p.ldo, p.Cpad, total);
  else if (p.taps == 25)
    hipLaunchKernelGGL((repvgg_stem_kernel<C0, 25>), dim3(grid), dim3(256), 0, s, p.feats, p.T, p.F, p.w, p.bias, p.out,
                       p.ldo, p.Cpad, total);
  else
    hipLaunchKernelGGL((repvgg_stem_kernel<C0, kRsbbLiveTaps>), dim3(grid), dim3(256), 0, s, p.feats, p.T, p.F, p.w,
                       p.bias, p.out, p.ldo, p.Cpad, total);
  WSP_HIP(hipGetLastError());
}

}  // namespace

void launch_rsbb_conv(const RsbbConvArgs& a, hipStream_t s) {
  WSP_CHECK(a.B > 0 && a.Fi > 0 && a.Ti > 0, "rsbb_conv: empty shape");
  WSP_CHECK(a.stride == 1 || a.stride == 2, "rsbb_conv: stride must be 1 or 2");
  WSP_CHECK(a.cin > 0 && a.cin % 32 == 0, "rsbb_conv: cin must be a multiple of 32");
  WSP_CHECK(a.N > 0 && a.N % 32 == 0, "rsbb_conv: N must be a multiple of 32");
  WSP_CHECK(a.ldx >= a.cin && a.ldx % 4 == 0 && reinterpret_cast<uintptr_t>(a.x) % 16 == 0,
            "rsbb_conv: input rows must be 16-byte aligned (ldx % 4 == 0, ldx >= cin)");
  WSP_CHECK(a.ldo >= a.N && a.ldo % 4 == 0 && reinterpret_cast<uintptr_t>(a.out) % 16 == 0,
            "rsbb_conv: output rows must be 16-byte aligned (ldo % 4 == 0, ldo >= N)");
  const int Fo = (a.Fi - 1) / a.stride + 1, To = (a.Ti - 1) / a.stride + 1;
  const long long M = (long long)a.B * Fo * To;
  const int K = kRsbbLiveTaps * a.cin, Kp = (K + 63) / 64 * 64;
  // buffer-load byte offsets are 32-bit: every operand stays below 2 GiB
  WSP_CHECK((long long)a.B * a.Fi * a.Ti * a.ldx * 4 < (long long)kOOB, "rsbb_conv: input exceeds 2 GiB (split the batch)");
  WSP_CHECK(M * a.ldo * 4 < (long long)kOOB, "rsbb_conv: output exceeds 2 GiB (split the batch)");
  WSP_CHECK((long long)a.N * Kp * 2 < (long long)kOOB, "rsbb_conv: weights exceed 2 GiB");
  ConvGemmArgs g{};
  g.a[0] = g.a[1] = g.a[2] = a.x;
  g.lda[0] = g.lda[1] = g.lda[2] = a.ldx;
  g.cseg[1] = g.cseg[2] = g.cseg[3] = a.cin;
  g.cin = a.cin;
  g.taps = kRsbbLiveTaps;
  g.dil = 1;
  g.pad = 2;
  g.M = (int)M;
  g.T = (int)M;
  g.N = a.N;
  g.K = K;
  g.Kp = Kp;
  g.bias = a.bias;
  g.out = a.out;
  g.ldo = a.ldo;
  g.act = kActRelu;
  g.conv2d = 1;
  g.Fi = a.Fi;
  g.Ti = a.Ti;
  g.Fo = Fo;
  g.To = To;
  g.stride = a.stride;
  g.kw = 5;
  if (a.N % 128 == 0)
    launch_rsbb_k<4>(g, a.whi, a.wlo, s);
  else if (a.N % 64 == 0)
    launch_rsbb_k<2>(g, a.whi, a.wlo, s);
  else
    launch_rsbb_k<1>(g, a.whi, a.wlo, s);
}

void launch_repvgg_stem(const RepvggStemArgs& p, hipStream_t s) {
  WSP_CHECK(p.C0 == 32 || p.C0 == 48 || p.C0 == 64, "repvgg stem: C0 must be 32, 48 or 64");
  WSP_CHECK(p.taps == 9 || p.taps == kRsbbLiveTaps || p.taps == 25, "repvgg stem: 9, 17 or 25 taps");
  WSP_CHECK(p.Cpad >= p.C0 && p.Cpad % 4 == 0 && p.ldo >= p.Cpad && p.ldo % 4 == 0 &&
                reinterpret_cast<uintptr_t>(p.out) % 16 == 0,
            "repvgg stem: output rows must be 16-byte aligned (C0 <= Cpad <= ldo, Cpad % 4 == 0, ldo % 4 == 0)");
  WSP_CHECK(p.B >= 0 && p.T > 0 && p.F > 0, "repvgg stem: bad shape");
  const long total = (long)p.B * p.F * p.T;
  if (total == 0) return;
  WSP_CHECK(total < (1L << 31), "repvgg stem: too many positions");
  if (p.C0 == 32)
    launch_stem_c<32>(p, total, s);
  else if (p.C0 == 48)
    launch_stem_c<48>(p, total, s);
  else
    launch_stem_c<64>(p, total, s);
}

}  // namespace wsp
