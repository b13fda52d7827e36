// ReDimNet kernels (interfaces and layout: redimnet.h).  Every kernel here is bound by the traffic
// of the [rows][1152] activation or by launch count, not by arithmetic (about 6 MMAC per frame in
// all), so each one is a whole block of the network: one read and one write of the activation, the
// intermediates in LDS, f32 fmaf chains.  Reductions (LayerNorm, softmax) run in a fixed order per
// row, so a row's result does not depend on its batch.
#include "redimnet.h"

#include "common.h"

namespace wsp {

namespace {

constexpr int kW = kRdWidth;
constexpr int kColThreads = 384;  // 3 columns of a 1152-wide row per thread
constexpr int kColsPer = kW / kColThreads;

__device__ __forceinline__ float4 ld4(const float* p) { return *reinterpret_cast<const float4*>(p); }
__device__ __forceinline__ void st4(float* p, float4 v) { *reinterpret_cast<float4*>(p) = v; }

// acc[r] = bias[co] + sum_k wt[k][co] * xs[r][g0 + k] for the group of gw columns that holds j
template <int R>
__device__ __forceinline__ void row_local(const float (*xs)[kW], int j, int gw, const float* __restrict__ wt,
                                          const float* __restrict__ bias, float (&acc)[R]) {
  const int g0 = j / gw * gw, co = j - g0;
  const float b = bias[co];
#pragma unroll
  for (int r = 0; r < R; ++r) acc[r] = b;
  const float* w = wt + co;
  for (int k = 0; k < gw; k += 4) {
    const float w0 = w[(size_t)k * gw], w1 = w[(size_t)(k + 1) * gw], w2 = w[(size_t)(k + 2) * gw],
                w3 = w[(size_t)(k + 3) * gw];
#pragma unroll
    for (int r = 0; r < R; ++r) {
      const float4 x = ld4(&xs[r][g0 + k]);
      acc[r] = fmaf(x.w, w3, fmaf(x.z, w2, fmaf(x.y, w1, fmaf(x.x, w0, acc[r]))));
    }
  }
}

// ------------------------------------------------------------------ stem ---
__global__ __launch_bounds__(256) void rd_stem_kernel(RdStemArgs p) {
  const long idx = (long)blockIdx.x * 256 + threadIdx.x;
  const long total = (long)p.B * p.T * p.F;
  if (idx >= total) return;
  const int f = (int)(idx % p.F);
  const long row = idx / p.F;
  const int t = (int)(row % p.T);
  float x[9];
#pragma unroll
  for (int kf = 0; kf < 3; ++kf)
#pragma unroll
    for (int kt = 0; kt < 3; ++kt) {
      const int ff = f + kf - 1, tt = t + kt - 1;
      x[kf * 3 + kt] = (ff >= 0 && ff < p.F && tt >= 0 && tt < p.T) ? p.feats[(row + kt - 1) * p.F + ff] : 0.f;
    }
  float y[16];
  float mean = 0.f;
#pragma unroll
  for (int c = 0; c < 16; ++c) {
    float a = p.bias[c];
#pragma unroll
    for (int tap = 0; tap < 9; ++tap) a = fmaf(x[tap], p.w[tap * 16 + c], a);
    y[c] = a;
    mean += a;
  }
  mean *= (1.f / 16.f);
  float var = 0.f;
#pragma unroll
  for (int c = 0; c < 16; ++c) {
    y[c] -= mean;
    var = fmaf(y[c], y[c], var);
  }
  const float rstd = 1.f / sqrtf(var * (1.f / 16.f) + p.eps);
  float* o = p.out + row * p.ldo + f * 16;
#pragma unroll
  for (int c = 0; c < 16; c += 4)
    st4(o + c, make_float4(fmaf(y[c] * rstd, p.gamma[c], p.beta[c]), fmaf(y[c + 1] * rstd, p.gamma[c + 1], p.beta[c + 1]),
                           fmaf(y[c + 2] * rstd, p.gamma[c + 2], p.beta[c + 2]),
                           fmaf(y[c + 3] * rstd, p.gamma[c + 3], p.beta[c + 3])));
}

// ----------------------------------------------------------- stage entry ---
constexpr int kEntryRows = 4;

__global__ __launch_bounds__(kColThreads) void rd_entry_kernel(RdEntryArgs p) {
  __shared__ __attribute__((aligned(16))) float xs[kEntryRows][kW];
  const int row0 = blockIdx.x * kEntryRows;
#pragma unroll
  for (int i = 0; i < kColsPer; ++i) {
    const int j = threadIdx.x + i * kColThreads;
    float a[kEntryRows];
#pragma unroll
    for (int r = 0; r < kEntryRows; ++r) a[r] = 0.f;
    for (int n = 0; n < p.n; ++n) {
      const float w = p.sw[n * kW + j];
      const float* in = p.in[n];
#pragma unroll
      for (int r = 0; r < kEntryRows; ++r)
        if (row0 + r < p.rows) a[r] = fmaf(w, in[(size_t)(row0 + r) * p.ld_in + j], a[r]);
    }
    if (p.gw == 0) {
#pragma unroll
      for (int r = 0; r < kEntryRows; ++r)
        if (row0 + r < p.rows) p.out[(size_t)(row0 + r) * p.ldo + j] = a[r];
    } else {
#pragma unroll
      for (int r = 0; r < kEntryRows; ++r) xs[r][j] = a[r];
    }
  }
  if (p.gw == 0) return;
  __syncthreads();
#pragma unroll
  for (int i = 0; i < kColsPer; ++i) {
    const int j = threadIdx.x + i * kColThreads;
    float acc[kEntryRows];
    row_local<kEntryRows>(xs, j, p.gw, p.wt, p.bias, acc);
#pragma unroll
    for (int r = 0; r < kEntryRows; ++r)
      if (row0 + r < p.rows) p.out[(size_t)(row0 + r) * p.ldo + j] = acc[r];
  }
}

// ------------------------------------------------------ 2-D ConvNeXt block ---
constexpr int kB2Rows = 4;  // output frames per block; the input tile has one halo frame on each side

__global__ __launch_bounds__(kColThreads) void rd_block2d_kernel(RdBlock2dArgs p) {
  __shared__ __attribute__((aligned(16))) float xin[kB2Rows + 2][kW];
  __shared__ __attribute__((aligned(16))) float mid[kB2Rows][kW];
  const int b = blockIdx.y, t0 = blockIdx.x * kB2Rows, c = p.c;
  const float* xb = p.x + (size_t)b * p.T * p.ldx;
  for (int i = threadIdx.x; i < (kB2Rows + 2) * (kW / 4); i += kColThreads) {
    const int r = i / (kW / 4), j4 = i - r * (kW / 4), t = t0 + r - 1;
    st4(&xin[r][j4 * 4], (t >= 0 && t < p.T) ? ld4(xb + (size_t)t * p.ldx + j4 * 4) : make_float4(0.f, 0.f, 0.f, 0.f));
  }
  __syncthreads();
#pragma unroll
  for (int i = 0; i < kColsPer; ++i) {
    const int j = threadIdx.x + i * kColThreads;
    const int f = j / c, co = j - f * c, g4 = co & ~3;
    float acc[kB2Rows];
    const float bd = p.bd[co];
#pragma unroll
    for (int r = 0; r < kB2Rows; ++r) acc[r] = bd;
#pragma unroll
    for (int kf = 0; kf < 3; ++kf) {
      const int ff = f + kf - 1;
      if (ff < 0 || ff >= p.F) continue;
      const int col = ff * c + g4;
#pragma unroll
      for (int kt = 0; kt < 3; ++kt) {
        const float* w = p.wd + (size_t)((kf * 3 + kt) * 4) * c + co;
        const float w0 = w[0], w1 = w[c], w2 = w[2 * c], w3 = w[3 * c];
#pragma unroll
        for (int r = 0; r < kB2Rows; ++r) {
          const float4 x = ld4(&xin[r + kt][col]);
          acc[r] = fmaf(x.w, w3, fmaf(x.z, w2, fmaf(x.y, w1, fmaf(x.x, w0, acc[r]))));
        }
      }
    }
#pragma unroll
    for (int r = 0; r < kB2Rows; ++r) mid[r][j] = gelu_as(acc[r]);
  }
  __syncthreads();
  float* ob = p.out + (size_t)b * p.T * p.ldo;
#pragma unroll
  for (int i = 0; i < kColsPer; ++i) {
    const int j = threadIdx.x + i * kColThreads;
    float acc[kB2Rows];
    row_local<kB2Rows>(mid, j, c, p.wp, p.bp, acc);
#pragma unroll
    for (int r = 0; r < kB2Rows; ++r)
      if (t0 + r < p.T) ob[(size_t)(t0 + r) * p.ldo + j] = acc[r] + xin[r + 1][j];
  }
}

// ------------------------------------------------------ 1-D ConvNeXt block ---
constexpr int kB1Rows = 8;
constexpr int kB1MaxC = 320;

__global__ void rd_block1d_kernel(RdBlock1dArgs p) {
  __shared__ __attribute__((aligned(16))) float mid[kB1Rows][kB1MaxC];
  const int b = blockIdx.y, t0 = blockIdx.x * kB1Rows, C = p.C, half = p.k / 2;
  const float* xb = p.x + (size_t)b * p.T * p.ldx;
  for (int i = threadIdx.x; i < kB1Rows * C; i += blockDim.x) {
    const int r = i / C, ch = i - r * C, t = t0 + r;
    float v = 0.f;
    if (t < p.T) {
      float a = p.bd[ch];
      const int lo = max(0, half - t), hi = min(p.k, p.T + half - t);  // taps whose frame t + kk - half is in [0, T)
      for (int kk = lo; kk < hi; ++kk) a = fmaf(p.wd[kk * C + ch], xb[(size_t)(t + kk - half) * p.ldx + ch], a);
      v = gelu_as(a);
    }
    mid[r][ch] = v;
  }
  __syncthreads();
  const int co = threadIdx.x;
  if (co >= C) return;
  float acc[kB1Rows];
  const float bp = p.bp[co];
#pragma unroll
  for (int r = 0; r < kB1Rows; ++r) acc[r] = bp;
  const float* w = p.wp + co;
  for (int k = 0; k < C; k += 4) {
    const float w0 = w[(size_t)k * C], w1 = w[(size_t)(k + 1) * C], w2 = w[(size_t)(k + 2) * C], w3 = w[(size_t)(k + 3) * C];
#pragma unroll
    for (int r = 0; r < kB1Rows; ++r) {
      const float4 x = ld4(&mid[r][k]);
      acc[r] = fmaf(x.w, w3, fmaf(x.z, w2, fmaf(x.y, w1, fmaf(x.x, w0, acc[r]))));
    }
  }
  float* ob = p.out + (size_t)b * p.T * p.ldo;
#pragma unroll
  for (int r = 0; r < kB1Rows; ++r)
    if (t0 + r < p.T) ob[(size_t)(t0 + r) * p.ldo + co] = acc[r] + xb[(size_t)(t0 + r) * p.ldx + co];
}

// --------------------------------------------------------------- LayerNorm ---
constexpr int kLnPer = 8;  // D <= 64 * 8

__global__ __launch_bounds__(256) void rd_ln_kernel(RdLnArgs p) {
  const int m = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (m >= p.M) return;
  const float* x = p.x + (size_t)m * p.ldx;
  const float* a = p.add ? p.add + (size_t)m * p.ldadd : nullptr;
  float v[kLnPer];
  float sum = 0.f;
#pragma unroll
  for (int i = 0; i < kLnPer; ++i) {
    const int d = lane + 64 * i;
    v[i] = d < p.D ? (a ? x[d] + a[d] : x[d]) : 0.f;
    sum += v[i];
  }
  const float mean = wave_sum(sum) / (float)p.D;
  float sq = 0.f;
#pragma unroll
  for (int i = 0; i < kLnPer; ++i) {
    const int d = lane + 64 * i;
    v[i] = d < p.D ? v[i] - mean : 0.f;
    sq = fmaf(v[i], v[i], sq);
  }
  const float rstd = 1.f / sqrtf(wave_sum(sq) / (float)p.D + p.eps);
  float* o = p.out + (size_t)m * p.ldo;
#pragma unroll
  for (int i = 0; i < kLnPer; ++i) {
    const int d = lane + 64 * i;
    if (d < p.D) o[d] = fmaf(v[i] * rstd, p.gamma[d], p.beta[d]);
  }
}

// --------------------------------------------------------------- attention ---
constexpr int kAtQ = 128;  // queries per block, one per thread
constexpr int kAtKC = 32;  // keys per LDS chunk
constexpr int kAtJS = 8;   // keys per running-maximum step

template <int DH>
__global__ __launch_bounds__(kAtQ) void rd_attn_kernel(RdAttnArgs p) {
  __shared__ __attribute__((aligned(16))) float Ks[kAtKC][DH];
  __shared__ __attribute__((aligned(16))) float Vs[kAtKC][DH];
  const int b = blockIdx.z, h = blockIdx.y, D = p.H * DH;
  const int tq = blockIdx.x * kAtQ + threadIdx.x;
  const float* base = p.qkv + (size_t)b * p.T * p.ld;
  float q[DH], acc[DH];
  {
    const float* qp = base + (size_t)min(tq, p.T - 1) * p.ld + h * DH;
#pragma unroll
    for (int d = 0; d < DH; d += 4) {
      const float4 v = ld4(qp + d);
      q[d] = v.x * p.scale, q[d + 1] = v.y * p.scale, q[d + 2] = v.z * p.scale, q[d + 3] = v.w * p.scale;
      acc[d] = acc[d + 1] = acc[d + 2] = acc[d + 3] = 0.f;
    }
  }
  float m = -INFINITY, l = 0.f;
  for (int k0 = 0; k0 < p.T; k0 += kAtKC) {
    const int nk = min(kAtKC, p.T - k0);
    __syncthreads();  // the previous chunk is consumed
    for (int i = threadIdx.x; i < kAtKC * (DH / 4); i += kAtQ) {
      const int j = i / (DH / 4), d = (i - j * (DH / 4)) * 4;
      float4 kv = make_float4(0.f, 0.f, 0.f, 0.f), vv = kv;
      if (j < nk) {
        const float* row = base + (size_t)(k0 + j) * p.ld + h * DH + d;
        kv = ld4(row + D);
        vv = ld4(row + 2 * D);
      }
      st4(&Ks[j][d], kv);
      st4(&Vs[j][d], vv);
    }
    __syncthreads();
    for (int js = 0; js < nk; js += kAtJS) {
      float sc[kAtJS];
      float cm = -INFINITY;
#pragma unroll
      for (int jj = 0; jj < kAtJS; ++jj) {
        float s = 0.f;
#pragma unroll
        for (int d = 0; d < DH; d += 4) {
          const float4 kv = ld4(&Ks[js + jj][d]);
          s = fmaf(q[d + 3], kv.w, fmaf(q[d + 2], kv.z, fmaf(q[d + 1], kv.y, fmaf(q[d], kv.x, s))));
        }
        sc[jj] = js + jj < nk ? s : -INFINITY;
        cm = fmaxf(cm, sc[jj]);
      }
      const float mn = fmaxf(m, cm);  // finite: key js is in range
      const float alpha = expf(m - mn);  // 0 on the first step (m = -inf)
      l *= alpha;
#pragma unroll
      for (int d = 0; d < DH; ++d) acc[d] *= alpha;
#pragma unroll
      for (int jj = 0; jj < kAtJS; ++jj) {
        const float pj = expf(sc[jj] - mn);  // 0 for the keys past nk (whose V rows are zero)
        l += pj;
#pragma unroll
        for (int d = 0; d < DH; d += 4) {
          const float4 vv = ld4(&Vs[js + jj][d]);
          acc[d] = fmaf(pj, vv.x, acc[d]);
          acc[d + 1] = fmaf(pj, vv.y, acc[d + 1]);
          acc[d + 2] = fmaf(pj, vv.z, acc[d + 2]);
          acc[d + 3] = fmaf(pj, vv.w, acc[d + 3]);
        }
      }
      m = mn;
    }
  }
  if (tq >= p.T) return;
  const float inv = 1.f / l;
  float* o = p.out + ((size_t)b * p.T + tq) * p.ldo + h * DH;
#pragma unroll
  for (int d = 0; d < DH; d += 4) st4(o + d, make_float4(acc[d] * inv, acc[d + 1] * inv, acc[d + 2] * inv, acc[d + 3] * inv));
}

// ---------------------------------------------------------------- NewGELU ---
__global__ __launch_bounds__(256) void rd_gelu_tanh_kernel(float* x, int ldx, int M, int D) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= (long)M * D) return;
  float* px = x + (i / D) * ldx + i % D;
  const float v = *px;
  *px = 0.5f * v * (1.f + tanhf(0.7978845608028654f * fmaf(0.044715f * v * v, v, v)));
}

bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

}  // namespace

void launch_rd_stem(const RdStemArgs& p, hipStream_t s) {
  WSP_CHECK(p.B > 0 && p.T > 0 && p.F * 16 == kW, "rd_stem: feats must be [B][T][72]");
  WSP_CHECK(p.ldo >= kW && p.ldo % 4 == 0 && aligned16(p.out), "rd_stem: output stride / alignment");
  const long total = (long)p.B * p.T * p.F;
  hipLaunchKernelGGL(rd_stem_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, p);
  WSP_HIP(hipGetLastError());
}

void launch_rd_entry(const RdEntryArgs& p, hipStream_t s) {
  WSP_CHECK(p.rows > 0 && p.n >= 1 && p.n <= kRdMaxIn, "rd_entry: 1..7 inputs");
  WSP_CHECK(p.ld_in >= kW && p.ldo >= kW, "rd_entry: row strides");
  WSP_CHECK(p.gw == 0 || (p.gw % 4 == 0 && kW % p.gw == 0), "rd_entry: the group width must divide 1152");
  hipLaunchKernelGGL(rd_entry_kernel, dim3(ceil_div(p.rows, kEntryRows)), dim3(kColThreads), 0, s, p);
  WSP_HIP(hipGetLastError());
}

bool rd_block2d_supported(int F, int c) { return F > 0 && c >= 4 && c % 4 == 0 && F * c == kW; }

void launch_rd_block2d(const RdBlock2dArgs& p, hipStream_t s) {
  WSP_CHECK(rd_block2d_supported(p.F, p.c), "rd_block2d: F * c must be 1152 with c % 4 == 0");
  WSP_CHECK(p.B > 0 && p.T > 0 && p.x != p.out, "rd_block2d: empty batch or in-place call");
  WSP_CHECK(p.ldx >= kW && p.ldx % 4 == 0 && p.ldo >= kW && aligned16(p.x), "rd_block2d: row strides / alignment");
  hipLaunchKernelGGL(rd_block2d_kernel, dim3(ceil_div(p.T, kB2Rows), p.B), dim3(kColThreads), 0, s, p);
  WSP_HIP(hipGetLastError());
}

void launch_rd_block1d(const RdBlock1dArgs& p, hipStream_t s) {
  WSP_CHECK(p.C >= 4 && p.C <= kB1MaxC && p.C % 4 == 0, "rd_block1d: C must be a multiple of 4, at most 320");
  WSP_CHECK(p.k >= 1 && p.k <= 59 && p.k % 2 == 1, "rd_block1d: k must be odd, at most 59");
  WSP_CHECK(p.B > 0 && p.T > 0 && p.x != p.out && p.ldx >= p.C && p.ldo >= p.C, "rd_block1d: shape or in-place call");
  hipLaunchKernelGGL(rd_block1d_kernel, dim3(ceil_div(p.T, kB1Rows), p.B), dim3((p.C + 63) / 64 * 64), 0, s, p);
  WSP_HIP(hipGetLastError());
}

void launch_rd_layernorm(const RdLnArgs& p, hipStream_t s) {
  WSP_CHECK(p.M > 0 && p.D > 0 && p.D <= 64 * kLnPer, "rd_layernorm: D must be at most 512");
  WSP_CHECK(p.ldx >= p.D && p.ldo >= p.D && (!p.add || p.ldadd >= p.D), "rd_layernorm: row strides");
  hipLaunchKernelGGL(rd_ln_kernel, dim3(ceil_div(p.M, 4)), dim3(256), 0, s, p);
  WSP_HIP(hipGetLastError());
}

bool rd_attn_supported(int dh) { return dh == 24 || dh == 36 || dh == 72; }

void launch_rd_attn(const RdAttnArgs& p, hipStream_t s) {
  WSP_CHECK(rd_attn_supported(p.dh), "rd_attn: head size must be 24, 36 or 72");
  WSP_CHECK(p.B > 0 && p.T > 0 && p.H > 0 && p.B <= 65535 && p.H <= 65535, "rd_attn: bad shape");
  WSP_CHECK(p.ld >= 3 * p.H * p.dh && p.ld % 4 == 0 && p.ldo >= p.H * p.dh && p.ldo % 4 == 0 && aligned16(p.qkv) &&
                aligned16(p.out),
            "rd_attn: row strides / alignment");
  const dim3 grid(ceil_div(p.T, kAtQ), p.H, p.B);
  if (p.dh == 24) hipLaunchKernelGGL(rd_attn_kernel<24>, grid, dim3(kAtQ), 0, s, p);
  else if (p.dh == 36) hipLaunchKernelGGL(rd_attn_kernel<36>, grid, dim3(kAtQ), 0, s, p);
  else hipLaunchKernelGGL(rd_attn_kernel<72>, grid, dim3(kAtQ), 0, s, p);
  WSP_HIP(hipGetLastError());
}

void launch_rd_gelu_tanh(float* x, int ldx, int M, int D, hipStream_t s) {
  WSP_CHECK(M > 0 && D > 0 && ldx >= D, "rd_gelu_tanh: bad shape");
  hipLaunchKernelGGL(rd_gelu_tanh_kernel, dim3((unsigned)(((long)M * D + 255) / 256)), dim3(256), 0, s, x, ldx, M, D);
  WSP_HIP(hipGetLastError());
}

}  // namespace wsp
