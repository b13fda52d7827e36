// XI pooling and the valid-conv offset tables (xi_pool.h).
//
// XI is HBM-bound: it reads the logits and the activations once (2 x rows x C floats) and writes
// B x C.  One workgroup = one utterance x 256 channels; a lane owns 4 adjacent channels (16-byte
// loads, a wave reads 1 KiB of a row), the 4 waves split the frames, two frames of both tensors in
// flight per lane.  Per element: one f32 softplus, then f64 w = s^2, W += w, A += w x.
#include "xi_pool.h"

#include <cstdint>

namespace wsp {

namespace {
// torch.nn.Softplus(beta=1, threshold=20): z > 20 -> z, else log1p(exp(z)); exp(z <= 20) cannot
// overflow, and log1pf keeps the relative accuracy of exp(z) where it is tiny
__device__ __forceinline__ float softplus20(float z) { return z > 20.f ? z : log1pf(expf(z)); }

__global__ __launch_bounds__(256) void xi_pool_kernel(XiPoolArgs p) {
  __shared__ double sm[4][2][4][64];
  const int b = blockIdx.x;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int c = (blockIdx.y * 64 + lane) * 4;
  const bool ok = c < p.C;
  const int T = p.seg ? p.seg[b + 1] - p.seg[b] : p.T;
  const long row0 = p.seg ? (long)p.seg[b] : (long)b * p.T;
  double W[4] = {0.0, 0.0, 0.0, 0.0}, A[4] = {0.0, 0.0, 0.0, 0.0};
  if (ok) {
    const float* zb = p.z + row0 * p.ldz + c;
    const float* xb = p.x + row0 * p.ldx + c;
    auto ldz = [&](int t) { return *reinterpret_cast<const f32x4*>(zb + (long)t * p.ldz); };
    auto ldx = [&](int t) { return *reinterpret_cast<const f32x4*>(xb + (long)t * p.ldx); };
    auto step = [&](const f32x4& zv, const f32x4& xv) {
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const double sv = (double)softplus20(zv[k]);
        const double w = sv * sv;
        W[k] += w;
        A[k] = fma(w, (double)xv[k], A[k]);
      }
    };
    int t = wave;
    for (; t + 4 < T; t += 8) {
      const f32x4 z0 = ldz(t), x0 = ldx(t), z1 = ldz(t + 4), x1 = ldx(t + 4);
      step(z0, x0);
      step(z1, x1);
    }
    if (t < T) step(ldz(t), ldx(t));
  }
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    sm[wave][0][k][lane] = W[k];
    sm[wave][1][k][lane] = A[k];
  }
  __syncthreads();
  if (wave == 0 && ok) {
    const f32x4 lp = *reinterpret_cast<const f32x4*>(p.prior_logprec + c);
    const f32x4 pm = *reinterpret_cast<const f32x4*>(p.prior_mean + c);
    f32x4 phi;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const double Ws = ((sm[0][0][k][lane] + sm[1][0][k][lane]) + sm[2][0][k][lane]) + sm[3][0][k][lane];
      const double As = ((sm[0][1][k][lane] + sm[1][1][k][lane]) + sm[2][1][k][lane]) + sm[3][1][k][lane];
      const double w0 = exp((double)lp[k]);
      phi[k] = (float)(fma(w0, (double)pm[k], As) / (Ws + w0));
    }
    *reinterpret_cast<f32x4*>(p.out + (long)b * p.ldo + c) = phi;
  }
}

__global__ void valid_conv_offsets_kernel(const int* __restrict__ off, int n1, int4 shrink, int n, int* __restrict__ out) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= n1) return;
  const int o = off[b];
  const int sh[4] = {shrink.x, shrink.y, shrink.z, shrink.w};
  for (int k = 0; k < n; ++k) out[k * n1 + b] = o - b * sh[k];
}
}  // namespace

void launch_xi_pool(const XiPoolArgs& p, hipStream_t s) {
  if (p.B == 0) return;
  WSP_CHECK(p.C > 0 && p.C % 4 == 0 && p.ldz % 4 == 0 && p.ldx % 4 == 0 && p.ldo % 4 == 0 && p.ldz >= p.C &&
                p.ldx >= p.C && p.ldo >= p.C,
            "xi_pool: C and the leading dimensions must be multiples of 4, ld >= C");
  WSP_CHECK(((reinterpret_cast<uintptr_t>(p.z) | reinterpret_cast<uintptr_t>(p.x) | reinterpret_cast<uintptr_t>(p.out) |
              reinterpret_cast<uintptr_t>(p.prior_mean) | reinterpret_cast<uintptr_t>(p.prior_logprec)) & 15) == 0,
            "xi_pool: operands must be 16-byte aligned");
  WSP_CHECK(p.seg || p.T >= 1, "xi_pool: needs T >= 1");
  const dim3 grid(p.B, (p.C + 255) / 256);
  hipLaunchKernelGGL(xi_pool_kernel, grid, dim3(256), 0, s, p);
  WSP_HIP(hipGetLastError());
}

void launch_valid_conv_offsets(const int* off, int B, const int* shrink, int n, int* out, hipStream_t s) {
  WSP_CHECK(B >= 1 && n >= 1 && n <= 4, "valid_conv_offsets: needs B >= 1 and 1..4 tables");
  int4 sh = {0, 0, 0, 0};
  int* v[4] = {&sh.x, &sh.y, &sh.z, &sh.w};
  for (int k = 0; k < n; ++k) *v[k] = shrink[k];
  hipLaunchKernelGGL(valid_conv_offsets_kernel, dim3((B + 1 + 255) / 256), dim3(256), 0, s, off, B + 1, sh, n, out);
  WSP_HIP(hipGetLastError());
}

}  // namespace wsp
