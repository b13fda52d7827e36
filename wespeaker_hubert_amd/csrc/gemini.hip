// Gemini DF-ResNet kernels (gemini_dfresnet.py:30-119; gemini.h has the contracts).
//
// The two MFMA kernels follow eres2net.hip: v_mfma_f32_16x16x32_bf16 with the weights as the A
// operand and 16 positions as the B operand's columns,
//
//   lane l holds A[row l & 15][k = 8 (l >> 4) .. + 7] and B[k = 8 (l >> 4) .. + 7][column l & 15];
//   accumulator register r is row 4 (l >> 4) + r, column l & 15,
//
// so a lane forms 8 consecutive input channels of one position per k-step and ends up with four
// consecutive output channels of that position (16-byte I/O throughout).  Weight fragments
// (pack::frag16) come straight from global memory: at most 1.2 MB, resident in L2.
//
// gemini_tail_kernel forms its B fragments from the depthwise conv: a lane's 8 channels of k-step
// ks are 8 independent 9-tap fmaf chains over the 3x3 neighbourhood of its position, read directly
// from global memory (no LDS, no barrier).  A y1 value is read by up to nine positions; six of the
// nine sit in the same or the neighbouring 16-position run of one wave (t - 1, t, t + 1 of three
// frequency rows), so the repeats hit L1 / L2 and HBM sees y1 once.  An LDS image of the tile
// would need a halo of a whole frequency row on either side (T' = 100 .. 200 positions for 16 .. 32
// owned) and a barrier per k-step group; the direct form keeps the kernel as simple as eres_conv.
#include "gemini.h"

#include "bf16x3.h"
#include "gemm_common.h"

namespace wsp {

namespace {

__device__ __forceinline__ void store4(__amdgpu_buffer_rsrc_t r, const f32x4 y, int off) {
  __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4, y), r, off, 0, 0);
}

// One output of the depthwise conv's arithmetic, shared by both kernels: 4 channels, tap `tap`.
__device__ __forceinline__ void dw_tap(f32x4& acc, const f32x4 w, const f32x4 y) {
#pragma unroll
  for (int e = 0; e < 4; ++e) acc[e] = fmaf(w[e], y[e], acc[e]);
}
__device__ __forceinline__ f32x4 dw_finish(const f32x4 acc, const f32x4 b) {
  f32x4 h;
#pragma unroll
  for (int e = 0; e < 4; ++e) h[e] = fmaxf(acc[e] + b[e], 0.f);
  return h;
}

// ------------------------------------------------------------------- depthwise 3x3 --
// One thread = 4 channels of kDwRun consecutive frames of one frequency row; consecutive threads
// walk the channels.  The three input rows are loaded once for the run (3 x (kDwRun + 2) loads and
// 9 weight loads for kDwRun outputs, against 9 + 9 for one), then every output runs its own
// chain over taps 0..8.
constexpr int kDwRun = 4;

__global__ __launch_bounds__(256) void gemini_dw_kernel(const GeminiDwArgs p, int runs_per_row, long long threads, int c4n) {
  const long long id = (long long)blockIdx.x * 256 + threadIdx.x;
  if (id >= threads) return;
  const int run = (int)(id / c4n);  // (b F + f) runs_per_row + run of the row
  const int c = 4 * (int)(id - (long long)run * c4n);
  const int bf = run / runs_per_row, t0 = (run - bf * runs_per_row) * kDwRun;
  const int b = bf / p.F, f = bf - b * p.F;
  const __amdgpu_buffer_rsrc_t ry = make_rsrc(p.y);
  f32x4 v[3][kDwRun + 2];
#pragma unroll
  for (int kf = 0; kf < 3; ++kf) {
    const int fi = f + kf - 1;
#pragma unroll
    for (int i = 0; i < kDwRun + 2; ++i) {
      const int ti = t0 + i - 1;
      const bool ok = fi >= 0 && fi < p.F && ti >= 0 && ti < p.T;
      v[kf][i] = bload4(ry, ok ? (((b * p.F + fi) * p.T + ti) * p.ldy + c) * 4 : kOOB);
    }
  }
  f32x4 acc[kDwRun];
#pragma unroll
  for (int j = 0; j < kDwRun; ++j) acc[j] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int tap = 0; tap < 9; ++tap) {
    const f32x4 w = *reinterpret_cast<const f32x4*>(p.w + tap * p.C + c);
#pragma unroll
    for (int j = 0; j < kDwRun; ++j) dw_tap(acc[j], w, v[tap / 3][j + tap % 3]);
  }
  const f32x4 bias = *reinterpret_cast<const f32x4*>(p.b + c);
#pragma unroll
  for (int j = 0; j < kDwRun; ++j)
    if (t0 + j < p.T)
      *reinterpret_cast<f32x4*>(p.out + ((size_t)bf * p.T + t0 + j) * p.ldo + c) = dw_finish(acc[j], bias);
}

// ---------------------------------------------------------------- bottleneck tail --
// One block = 4 waves; a wave owns PT x 16 positions and NT x 16 output channels (blockIdx.y
// selects the channel group when d / 16 > NT).
template <int NT, int PT>
__global__ __launch_bounds__(256) void gemini_tail_kernel(const GeminiTailArgs p, int M) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int r16 = lane & 15, qk = lane >> 4;
  const int m0 = (blockIdx.x * 4 + wave) * (16 * PT);
  if (m0 >= M) return;  // wave-uniform; the kernel has no barrier
  const int jt0 = blockIdx.y * NT, tiles = p.d / 16, K = 4 * p.d;
  const __amdgpu_buffer_rsrc_t ry = make_rsrc(p.y1);
  int row0[PT], f0[PT], t0[PT];
  bool live[PT];
#pragma unroll
  for (int pt = 0; pt < PT; ++pt) {
    const int m = m0 + 16 * pt + r16;
    live[pt] = m < M;
    const int mm = live[pt] ? m : 0;
    const int b = mm / (p.F * p.T), rem = mm - b * p.F * p.T;
    f0[pt] = rem / p.T;
    t0[pt] = rem - f0[pt] * p.T;
    row0[pt] = b * p.F * p.T;
  }
  const uint4* wsrc = reinterpret_cast<const uint4*>(p.w3);
  f32x4 acc[PT][NT];
#pragma unroll
  for (int pt = 0; pt < PT; ++pt)
#pragma unroll
    for (int j = 0; j < NT; ++j) acc[pt][j] = f32x4{0.f, 0.f, 0.f, 0.f};

  for (int ks = 0; ks < K / 32; ++ks) {
    const int c = 32 * ks + 8 * qk;  // this lane's 8 channels of h
    f32x4 h[PT][2];
#pragma unroll
    for (int pt = 0; pt < PT; ++pt) h[pt][0] = h[pt][1] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int tap = 0; tap < 9; ++tap) {
      const f32x4 w0 = *reinterpret_cast<const f32x4*>(p.w2 + tap * K + c);
      const f32x4 w1 = *reinterpret_cast<const f32x4*>(p.w2 + tap * K + c + 4);
#pragma unroll
      for (int pt = 0; pt < PT; ++pt) {
        const int fi = f0[pt] + tap / 3 - 1, ti = t0[pt] + tap % 3 - 1;
        const bool ok = live[pt] && fi >= 0 && fi < p.F && ti >= 0 && ti < p.T;
        const int off = ok ? ((row0[pt] + fi * p.T + ti) * p.ldy + c) * 4 : kOOB;
        dw_tap(h[pt][0], w0, bload4(ry, off));
        dw_tap(h[pt][1], w1, bload4(ry, ok ? off + 16 : kOOB));
      }
    }
    const f32x4 b0 = *reinterpret_cast<const f32x4*>(p.b2 + c);
    const f32x4 b1 = *reinterpret_cast<const f32x4*>(p.b2 + c + 4);
    bf16x8 bh[PT], bl[PT];
#pragma unroll
    for (int pt = 0; pt < PT; ++pt) {
      const f32x4 u0 = dw_finish(h[pt][0], b0), u1 = dw_finish(h[pt][1], b1);
      const float v[8] = {u0[0], u0[1], u0[2], u0[3], u1[0], u1[1], u1[2], u1[3]};
      split(v, bh[pt], bl[pt]);
    }
#pragma unroll
    for (int j = 0; j < NT; ++j) {
      const bf16x8 wh = __builtin_bit_cast(bf16x8, wsrc[((size_t)(ks * 2 + 0) * tiles + jt0 + j) * 64 + lane]);
      const bf16x8 wl = __builtin_bit_cast(bf16x8, wsrc[((size_t)(ks * 2 + 1) * tiles + jt0 + j) * 64 + lane]);
#pragma unroll
      for (int pt = 0; pt < PT; ++pt) mma3(wh, wl, bh[pt], bl[pt], acc[pt][j]);
    }
  }

  // ---- epilogue: bias + residual, ReLU, 16-byte stores of 4 channels (launch_eres_pw's order)
  const __amdgpu_buffer_rsrc_t ro = make_rsrc(p.out);
  const __amdgpu_buffer_rsrc_t rr = make_rsrc(p.res);
#pragma unroll
  for (int j = 0; j < NT; ++j) {
    const int c = (jt0 + j) * 16 + 4 * qk;
    const f32x4 bv = *reinterpret_cast<const f32x4*>(p.b3 + c);
#pragma unroll
    for (int pt = 0; pt < PT; ++pt) {
      const int m = m0 + 16 * pt + r16;
      const bool ok = m < M;
      f32x4 y = acc[pt][j] + bv;
      y += bload4(rr, ok ? (m * p.ldres + c) * 4 : kOOB);
#pragma unroll
      for (int e = 0; e < 4; ++e) y[e] = fmaxf(y[e], 0.f);
      store4(ro, y, ok ? (m * p.ldo + c) * 4 : kOOB);
    }
  }
}

// ------------------------------------------------------------------ downsample 3x3 --
struct DownGeom {
  int Fo, To, M, KS, tiles;
};

// The implicit GEMM over 9 taps x cin; the activations of a k-step are loaded one step ahead.
template <int NT, int PT>
__global__ __launch_bounds__(256) void gemini_down_kernel(const GeminiDownArgs p, const DownGeom g) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int r16 = lane & 15, qk = lane >> 4;
  const int m0 = (blockIdx.x * 4 + wave) * (16 * PT);
  if (m0 >= g.M) return;  // wave-uniform; the kernel has no barrier
  const int jt0 = blockIdx.y * NT;
  const __amdgpu_buffer_rsrc_t ra = make_rsrc(p.a);
  int ib[PT], fi0[PT], ti0[PT];
  bool live[PT];
#pragma unroll
  for (int pt = 0; pt < PT; ++pt) {
    const int m = m0 + 16 * pt + r16;
    live[pt] = m < g.M;
    const int mm = live[pt] ? m : 0;
    const int b = mm / (g.Fo * g.To), rem = mm - b * g.Fo * g.To;
    const int fo = rem / g.To, to = rem - fo * g.To;
    fi0[pt] = fo * p.sf - 1;
    ti0[pt] = to * p.st - 1;
    ib[pt] = b * p.Fi * p.Ti;
  }
  const uint4* wsrc = reinterpret_cast<const uint4*>(p.w);
  f32x4 acc[PT][NT];
#pragma unroll
  for (int pt = 0; pt < PT; ++pt)
#pragma unroll
    for (int j = 0; j < NT; ++j) acc[pt][j] = f32x4{0.f, 0.f, 0.f, 0.f};

  auto gload = [&](int ks, f32x4 (&v)[PT][2]) {
    // a lane's 8 consecutive k stay inside one tap (cin % 8 == 0); K = 9 cin is a multiple of 32
    const int k8 = 32 * ks + 8 * qk;
    const int tap = k8 / p.cin, c = k8 - tap * p.cin;
    const int kf = tap / 3, kt = tap - 3 * kf;
#pragma unroll
    for (int pt = 0; pt < PT; ++pt) {
      const int fi = fi0[pt] + kf, ti = ti0[pt] + kt;
      const bool ok = live[pt] && fi >= 0 && fi < p.Fi && ti >= 0 && ti < p.Ti;
      const int off = ok ? ((ib[pt] + fi * p.Ti + ti) * p.lda + c) * 4 : kOOB;
      v[pt][0] = bload4(ra, off);
      v[pt][1] = bload4(ra, ok ? off + 16 : kOOB);
    }
  };
  f32x4 v[PT][2];
  gload(0, v);
  for (int ks = 0; ks < g.KS; ++ks) {
    bf16x8 bh[PT], bl[PT];
#pragma unroll
    for (int pt = 0; pt < PT; ++pt) {
      const float u[8] = {v[pt][0][0], v[pt][0][1], v[pt][0][2], v[pt][0][3],
                          v[pt][1][0], v[pt][1][1], v[pt][1][2], v[pt][1][3]};
      split(u, bh[pt], bl[pt]);
    }
    if (ks + 1 < g.KS) gload(ks + 1, v);  // in flight under this step's MFMAs
#pragma unroll
    for (int j = 0; j < NT; ++j) {
      const bf16x8 wh = __builtin_bit_cast(bf16x8, wsrc[((size_t)(ks * 2 + 0) * g.tiles + jt0 + j) * 64 + lane]);
      const bf16x8 wl = __builtin_bit_cast(bf16x8, wsrc[((size_t)(ks * 2 + 1) * g.tiles + jt0 + j) * 64 + lane]);
#pragma unroll
      for (int pt = 0; pt < PT; ++pt) mma3(wh, wl, bh[pt], bl[pt], acc[pt][j]);
    }
  }
  const __amdgpu_buffer_rsrc_t ro = make_rsrc(p.out);
#pragma unroll
  for (int j = 0; j < NT; ++j) {
    const int c = (jt0 + j) * 16 + 4 * qk;
    const f32x4 bv = *reinterpret_cast<const f32x4*>(p.bias + c);
#pragma unroll
    for (int pt = 0; pt < PT; ++pt) {
      const int m = m0 + 16 * pt + r16;
      store4(ro, acc[pt][j] + bv, m < g.M ? (m * p.ldo + c) * 4 : kOOB);
    }
  }
}

bool aligned16(const void* q) { return (reinterpret_cast<uintptr_t>(q) & 15) == 0; }

template <int NT, int PT>
void launch_tail_nt(const GeminiTailArgs& p, int M, int ny, hipStream_t s) {
  const long long gx = ((long long)M + 64 * PT - 1) / (64 * PT);
  WSP_CHECK(gx < (1LL << 31), "gemini_tail: grid too large");
  hipLaunchKernelGGL((gemini_tail_kernel<NT, PT>), dim3((unsigned)gx, ny), dim3(256), 0, s, p, M);
  WSP_HIP(hipGetLastError());
}

template <int NT>
void launch_down_nt(const GeminiDownArgs& p, const DownGeom& g, hipStream_t s) {
  constexpr int PT = 2;
  const long long gx = ((long long)g.M + 64 * PT - 1) / (64 * PT);
  WSP_CHECK(gx < (1LL << 31), "gemini_down: grid too large");
  hipLaunchKernelGGL((gemini_down_kernel<NT, PT>), dim3((unsigned)gx, g.tiles / NT), dim3(256), 0, s, p, g);
  WSP_HIP(hipGetLastError());
}

}  // namespace

bool gemini_dw_supported(int C) { return C == 128 || C == 256 || C == 512 || C == 1024; }

void launch_gemini_dw(const GeminiDwArgs& p, hipStream_t s) {
  WSP_CHECK(p.B > 0 && p.F > 0 && p.T > 0 && gemini_dw_supported(p.C), "gemini_dw: C in {128, 256, 512, 1024}");
  WSP_CHECK(p.ldy >= p.C && p.ldy % 4 == 0 && p.ldo >= p.C && p.ldo % 4 == 0, "gemini_dw: bad strides");
  WSP_CHECK(p.y && p.w && p.b && p.out && aligned16(p.y) && aligned16(p.w) && aligned16(p.b) && aligned16(p.out),
            "gemini_dw: operands must be 16-byte aligned");
  const long long M = (long long)p.B * p.F * p.T;
  WSP_CHECK(M * p.ldy * 4 < (long long)kOOB && M * p.ldo * 4 < (long long)kOOB,
            "gemini_dw: operand exceeds 2 GiB (split the batch)");
  const int c4n = p.C / 4, runs_per_row = (p.T + kDwRun - 1) / kDwRun;
  const long long threads = (long long)p.B * p.F * runs_per_row * c4n, gx = (threads + 255) / 256;
  WSP_CHECK(gx < (1LL << 31), "gemini_dw: grid too large");
  hipLaunchKernelGGL(gemini_dw_kernel, dim3((unsigned)gx), dim3(256), 0, s, p, runs_per_row, threads, c4n);
  WSP_HIP(hipGetLastError());
}

bool gemini_tail_supported(int d) { return d == 32 || d == 64 || d == 128 || d == 256; }

void launch_gemini_tail(const GeminiTailArgs& p, hipStream_t s) {
  WSP_CHECK(p.B > 0 && p.F > 0 && p.T > 0 && gemini_tail_supported(p.d), "gemini_tail: d in {32, 64, 128, 256}");
  WSP_CHECK(p.ldy >= 4 * p.d && p.ldy % 4 == 0 && p.ldres >= p.d && p.ldres % 4 == 0 && p.ldo >= p.d && p.ldo % 4 == 0,
            "gemini_tail: bad strides");
  WSP_CHECK(p.y1 && p.w2 && p.b2 && p.w3 && p.b3 && p.res && p.out && aligned16(p.y1) && aligned16(p.w2) &&
                aligned16(p.b2) && aligned16(p.w3) && aligned16(p.b3) && aligned16(p.res) && aligned16(p.out),
            "gemini_tail: operands must be 16-byte aligned");
  WSP_CHECK(p.out != p.y1 && p.out != p.res, "gemini_tail: out aliases an input");
  const long long M = (long long)p.B * p.F * p.T;
  WSP_CHECK(M * p.ldy * 4 < (long long)kOOB && M * p.ldres * 4 < (long long)kOOB && M * p.ldo * 4 < (long long)kOOB,
            "gemini_tail: operand exceeds 2 GiB (split the batch)");
  // every output's k order is the same whatever the split, so the result does not depend on it
  switch (p.d) {
    case 32: return launch_tail_nt<2, 2>(p, (int)M, 1, s);
    case 64: return launch_tail_nt<4, 2>(p, (int)M, 1, s);
    case 128: return launch_tail_nt<8, 2>(p, (int)M, 1, s);
    default: return launch_tail_nt<8, 2>(p, (int)M, 2, s);  // 256: two channel groups, h formed in each
  }
}

bool gemini_down_supported(int cin, int N) {
  return (cin == 32 && N == 32) || (cin == 32 && N == 64) || (cin == 64 && N == 128) || (cin == 128 && N == 256);
}

void launch_gemini_down(const GeminiDownArgs& p, hipStream_t s) {
  WSP_CHECK(p.B > 0 && p.Fi > 0 && p.Ti > 0 && gemini_down_supported(p.cin, p.N),
            "gemini_down: (cin, N) in {(32, 32), (32, 64), (64, 128), (128, 256)}");
  WSP_CHECK(p.sf == 2 && (p.st == 1 || p.st == 2), "gemini_down: strides (2, 1) or (2, 2)");
  WSP_CHECK(p.lda >= p.cin && p.lda % 4 == 0 && p.ldo >= p.N && p.ldo % 4 == 0, "gemini_down: bad strides");
  WSP_CHECK(p.a && p.w && p.bias && p.out && aligned16(p.a) && aligned16(p.w) && aligned16(p.bias) && aligned16(p.out),
            "gemini_down: operands must be 16-byte aligned");
  DownGeom g;
  g.Fo = (p.Fi - 1) / p.sf + 1;
  g.To = (p.Ti - 1) / p.st + 1;
  const long long M = (long long)p.B * g.Fo * g.To, in_rows = (long long)p.B * p.Fi * p.Ti;
  WSP_CHECK(in_rows * p.lda * 4 < (long long)kOOB && M * p.ldo * 4 < (long long)kOOB,
            "gemini_down: operand exceeds 2 GiB (split the batch)");
  g.M = (int)M;
  g.KS = 9 * p.cin / 32;
  g.tiles = p.N / 16;
  switch (g.tiles) {
    case 2: return launch_down_nt<2>(p, g, s);
    case 4: return launch_down_nt<4>(p, g, s);
    default: return launch_down_nt<8>(p, g, s);  // 8 or 16 tiles: one or two channel groups
  }
}

}  // namespace wsp
