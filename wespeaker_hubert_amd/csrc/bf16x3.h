// bf16x3 split-precision products: an fp32 value x is carried as two bf16 terms, hi = bf16(x) and
// lo = bf16(x - hi), and a product x * y is the three MFMAs lo*hi + hi*lo + hi*hi (lo*lo is below
// fp32 resolution).  The vector types, the split and the MFMA triple, for the kernels
// that share them.
#pragma once

#include "common.h"

namespace wsp {

typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef __bf16 bf16x4 __attribute__((ext_vector_type(4)));
typedef unsigned u32x4 __attribute__((ext_vector_type(4)));

// fp32 -> bf16 hi / lo.  No fp-contract pragma here: whether `x - hi` may fuse with a multiply
// that produced x is the caller's choice.
__device__ __forceinline__ void split(const f32x4 x, bf16x4& hi, bf16x4& lo) {
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    const __bf16 h = (__bf16)x[e];
    hi[e] = h;
    lo[e] = (__bf16)(x[e] - (float)h);
  }
}
// 8 values
__device__ __forceinline__ void split(const float (&v)[8], bf16x8& hi, bf16x8& lo) {
#pragma unroll
  for (int e = 0; e < 8; ++e) {
    hi[e] = (__bf16)v[e];
    lo[e] = (__bf16)(v[e] - (float)hi[e]);
  }
}

// c += x * y in bf16x3, x the MFMA's A operand and y its B operand: xl*yh, then xh*yl, then
// xh*yh.  Each MFMA rounds into c, so the order is part of the result: every kernel issues this
// one, smallest terms first, and that is what makes the GEMM tile families bit-identical to each
// other (and a fused kernel to the unfused pair it replaces).  f32x4 accumulators take the
// 16x16x32 MFMA, f32x16 the 32x32x16 one.
__device__ __forceinline__ void mma3(const bf16x8 xh, const bf16x8 xl, const bf16x8 yh, const bf16x8 yl, f32x4& c) {
  c = __builtin_amdgcn_mfma_f32_16x16x32_bf16(xl, yh, c, 0, 0, 0);
  c = __builtin_amdgcn_mfma_f32_16x16x32_bf16(xh, yl, c, 0, 0, 0);
  c = __builtin_amdgcn_mfma_f32_16x16x32_bf16(xh, yh, c, 0, 0, 0);
}
__device__ __forceinline__ void mma3(const bf16x8 xh, const bf16x8 xl, const bf16x8 yh, const bf16x8 yl, f32x16& c) {
  c = __builtin_amdgcn_mfma_f32_32x32x16_bf16(xl, yh, c, 0, 0, 0);
  c = __builtin_amdgcn_mfma_f32_32x32x16_bf16(xh, yl, c, 0, 0, 0);
  c = __builtin_amdgcn_mfma_f32_32x32x16_bf16(xh, yh, c, 0, 0, 0);
}

}  // namespace wsp
