// CAM++ FCM head (campplus.py:245-330): Conv2d(32, 32, 3, stride (2, 1), padding 1) + folded
// BatchNorm (+ ReLU), optionally with the block's 1x1 stride-(2, 1) projection shortcut from the
// same fragments.  ConvGemmArgs::stride strides both axes, so the implicit GEMM cannot run these.
//
// An implicit GEMM over output positions (b, fo, t) with K = 9 taps x 32 channels: one 32-k
// MFMA step per tap, N = 32 (two 16-column tiles), bf16x3 products on 16x16x32 MFMAs.  The
// weights' fragment image (36 KB, + 4 KB for the shortcut) is staged in LDS once per block; a
// block walks kIters x 128 output positions, each wave 32 of them at a time, reading its A
// fragments straight from global memory (a tap outside the image reads zero through the
// buffer descriptor's range check).  The shortcut's input x[b][2 fo][t] is exactly the centre
// tap's fragment.
#include "fcm_conv.h"

#include "gemm_common.h"

namespace wsp {
namespace {

typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
constexpr int kIters = 4;
constexpr int kWChunks = 9 * 2 * 2 * 64, kScChunks = 2 * 2 * 64;  // 16-byte chunks

__global__ __launch_bounds__(256) void fcm_conv_kernel(const FcmConvArgs p, int Fo, int M) {
  __shared__ uint4 wl[kWChunks + kScChunks];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int r16 = lane & 15, qk = lane >> 4;
  {
    const uint4* src = reinterpret_cast<const uint4*>(p.w);
    for (int q = tid; q < kWChunks; q += 256) wl[q] = src[q];
    if (p.wsc) {
      const uint4* ssrc = reinterpret_cast<const uint4*>(p.wsc);
      for (int q = tid; q < kScChunks; q += 256) wl[kWChunks + q] = ssrc[q];
    }
  }
  __syncthreads();
  const __amdgpu_buffer_rsrc_t rx = make_rsrc(p.x);
  const __amdgpu_buffer_rsrc_t ro = make_rsrc(p.out);
  const __amdgpu_buffer_rsrc_t rs = make_rsrc(p.sc ? p.sc : p.out);
  const bool has_sc = p.wsc != nullptr;  // block-uniform

  for (int it = 0; it < kIters; ++it) {
    const int m0 = (blockIdx.x * kIters + it) * 128 + 32 * wave;
    if (m0 >= M) break;  // wave-uniform; no barrier below
    int ab[2], af[2], at[2];
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const int m = m0 + 16 * i + r16;
      const int mm = m < M ? m : 0;
      const int t = mm % p.T, q = mm / p.T;
      const int fo = q % Fo, b = q / Fo;
      ab[i] = b * p.Fi;
      af[i] = m < M ? 2 * fo - 1 : -0x40000000;
      at[i] = t - 1;
    }
    f32x4 acc[2][2], accs[2][2];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
      for (int j = 0; j < 2; ++j) acc[i][j] = accs[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int tap = 0; tap < 9; ++tap) {
      const int kf = tap / 3, kt = tap - 3 * kf;
      bf16x8 ah[2], al[2];
#pragma unroll
      for (int i = 0; i < 2; ++i) {
        const int fi = af[i] + kf, ti = at[i] + kt;
        const bool ok = fi >= 0 && fi < p.Fi && ti >= 0 && ti < p.T;
        const int off = ok ? (((ab[i] + fi) * p.T + ti) * 32 + 8 * qk) * 4 : kOOB;
        const f32x4 v0 = bload4(rx, off), v1 = bload4(rx, ok ? off + 16 : kOOB);
#pragma unroll
        for (int e = 0; e < 8; ++e) {
          const float v = e < 4 ? v0[e & 3] : v1[e & 3];
          ah[i][e] = (__bf16)v;
          al[i][e] = (__bf16)(v - (float)ah[i][e]);
        }
      }
#pragma unroll
      for (int j = 0; j < 2; ++j) {
        const bf16x8 bh = __builtin_bit_cast(bf16x8, wl[((tap * 2 + 0) * 2 + j) * 64 + lane]);
        const bf16x8 bl = __builtin_bit_cast(bf16x8, wl[((tap * 2 + 1) * 2 + j) * 64 + lane]);
#pragma unroll
        for (int i = 0; i < 2; ++i) {
          f32x4& c = acc[i][j];
          c = __builtin_amdgcn_mfma_f32_16x16x32_bf16(al[i], bh, c, 0, 0, 0);
          c = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ah[i], bl, c, 0, 0, 0);
          c = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ah[i], bh, c, 0, 0, 0);
        }
      }
      if (tap == 4 && has_sc) {
#pragma unroll
        for (int j = 0; j < 2; ++j) {
          const bf16x8 bh = __builtin_bit_cast(bf16x8, wl[kWChunks + (0 * 2 + j) * 64 + lane]);
          const bf16x8 bl = __builtin_bit_cast(bf16x8, wl[kWChunks + (1 * 2 + j) * 64 + lane]);
#pragma unroll
          for (int i = 0; i < 2; ++i) {
            f32x4& c = accs[i][j];
            c = __builtin_amdgcn_mfma_f32_16x16x32_bf16(al[i], bh, c, 0, 0, 0);
            c = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ah[i], bl, c, 0, 0, 0);
            c = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ah[i], bh, c, 0, 0, 0);
          }
        }
      }
    }
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int m = m0 + 16 * i + 4 * qk + r;
        const bool ok = m < M;
        int row = m;  // NHWC position index; tfc: frame rows [b][t][fo]
        if (p.tfc) {
          const int mm = ok ? m : 0;
          const int t = mm % p.T, q = mm / p.T;
          const int fo = q % Fo, b = q / Fo;
          row = (b * p.T + t) * Fo + fo;
        }
#pragma unroll
        for (int j = 0; j < 2; ++j) {
          const int col = 16 * j + r16;
          float y = acc[i][j][r] + p.bias[col];
          if (p.relu) y = fmaxf(y, 0.f);
          __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(unsigned, y), ro, ok ? (row * 32 + col) * 4 : kOOB,
                                                0, 0);
          if (has_sc) {
            const float z = accs[i][j][r] + p.bsc[col];
            __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(unsigned, z), rs, ok ? (m * 32 + col) * 4 : kOOB,
                                                  0, 0);
          }
        }
      }
  }
}

}  // namespace

void launch_fcm_conv(const FcmConvArgs& p, hipStream_t s) {
  WSP_CHECK(p.B > 0 && p.Fi >= 1 && p.T >= 1, "fcm_conv: empty input");
  WSP_CHECK((p.wsc == nullptr) == (p.sc == nullptr) && (p.wsc == nullptr) == (p.bsc == nullptr),
            "fcm_conv: the shortcut needs its weights, bias and output");
  WSP_CHECK(!(p.wsc && p.tfc), "fcm_conv: the shortcut is written in NHWC order only");
  WSP_CHECK((reinterpret_cast<uintptr_t>(p.x) & 15) == 0 && (reinterpret_cast<uintptr_t>(p.w) & 15) == 0 &&
                (reinterpret_cast<uintptr_t>(p.wsc) & 15) == 0,
            "fcm_conv: operands must be 16-byte aligned");
  const int Fo = (p.Fi - 1) / 2 + 1;
  const long long rows_in = (long long)p.B * p.Fi * p.T, M = (long long)p.B * Fo * p.T;
  WSP_CHECK(rows_in * 128 < (long long)kOOB, "fcm_conv: operand exceeds 2 GiB (split the batch)");
  const long long blocks = (M + 128 * kIters - 1) / (128 * kIters);
  hipLaunchKernelGGL(fcm_conv_kernel, dim3((unsigned)blocks), dim3(256), 0, s, p, Fo, (int)M);
  WSP_HIP(hipGetLastError());
}

}  // namespace wsp
