// CAM++ dense-TDNN layer kernels (campplus.py:86-170; cam_dense.h has the contracts).
//
// A CAMDenseTDNNLayer reads the whole growing concatenation x [M][cin] of its block, and the
// BatchNorm + ReLU in front of its 1x1 conv cannot be folded into the weights.  cam_gemm_kernel
// applies that affine + ReLU to the A operand as its fragments are read (one fma and one max per
// element, before the bf16 hi / lo split), so the concatenation is read once per layer and no
// normalised copy of it is ever written.  Its epilogue applies the layer's second BatchNorm +
// ReLU and emits the per-(utterance, 100-frame segment) column sums of h that the context mask
// needs; cam_mask_kernel turns them into the mask and cam_local_kernel runs the k3 dilated conv
// (N = 32) with the mask in its epilogue, writing straight into the block's dense buffer.
//
// MFMA operand layout (v_mfma_f32_16x16x32_bf16): lane l holds row / column l & 15 and the 8
// consecutive k 8 (l >> 4) .. + 7; accumulator register r is row 4 (l >> 4) + r, column l & 15.
#include "cam_dense.h"

#include "bf16x3.h"
#include "gemm_common.h"
#include "pack.h"

namespace wsp {

std::vector<uint16_t> cam_pack_b(const float* w, int N, int K, int ldw) {
  WSP_CHECK(N > 0 && K > 0 && N % 16 == 0 && K % 32 == 0 && ldw >= K, "cam_pack_b: N % 16, K % 32");
  const int KS = K / 32, NT = N / 16;
  std::vector<uint16_t> out((size_t)KS * 2 * NT * 64 * 8);
  for (int ks = 0; ks < KS; ++ks)
    for (int j = 0; j < NT; ++j)
      for (int l = 0; l < 64; ++l)
        for (int e = 0; e < 8; ++e) {
          const float v = w[(size_t)(16 * j + (l & 15)) * ldw + 32 * ks + 8 * (l >> 4) + e];
          const uint16_t hi = pack::f2bf(v);
          const uint16_t lo = pack::f2bf(v - pack::bf2f(hi));
          const size_t at = (((size_t)(ks * 2) * NT + j) * 64 + l) * 8 + e;
          out[at] = hi;
          out[at + (size_t)NT * 64 * 8] = lo;
        }
  return out;
}

namespace {

__device__ __forceinline__ void store1(__amdgpu_buffer_rsrc_t r, float y, int off) {
  __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(unsigned, y), r, off, 0, 0);
}

// ------------------------------------------------------------- BN-ReLU-prologue GEMM --
// One block = 128 rows x 128 columns, 4 waves of 32 rows x 128 columns (2 x 8 accumulators).
// The 32-k step of W (both planes, 16 KB) goes through a double-buffered LDS image that all four
// waves read; A fragments come straight from global memory (each wave owns its rows), one k-step
// ahead in registers.
constexpr int kGemmRows = 128, kGemmCols = 128, kStepBytes = 2 * 8 * 64 * 16;

__global__ __launch_bounds__(256) void cam_gemm_kernel(const CamGemmArgs p) {
  __shared__ __attribute__((aligned(16))) unsigned char smem[2][kStepBytes];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int r16 = lane & 15, qk = lane >> 4;
  int r0, nrows, strip = 0;
  if (p.segsum) {
    const int nseg = (p.T + kCamSeg - 1) / kCamSeg;
    strip = blockIdx.x;
    const int b = strip / nseg, sg = strip - b * nseg;
    r0 = b * p.T + sg * kCamSeg;
    nrows = min(kCamSeg, p.T - sg * kCamSeg);
  } else {
    r0 = blockIdx.x * kGemmRows;
    nrows = min(kGemmRows, p.M - r0);
  }
  const int n0 = blockIdx.y * kGemmCols;
  const int KS = p.K / 32, NT = p.N / 16;
  const __amdgpu_buffer_rsrc_t ra = make_rsrc(p.a);
  int abase[2];
  bool aok[2];
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    const int lr = 32 * wave + 16 * i + r16;
    aok[i] = lr < nrows;
    abase[i] = aok[i] ? ((r0 + lr) * p.lda + 8 * qk) * 4 : 0;  // dead rows: never formed (could pass 2^31)
  }
  const uint4* wsrc = reinterpret_cast<const uint4*>(p.w) + (size_t)blockIdx.y * 8 * 64;

  f32x4 araw[2][2], sraw[2], traw[2];
  uint4 braw[2][2];
  auto gload = [&](int ks) {
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const int off = aok[i] ? abase[i] + ks * 128 : kOOB;
      araw[i][0] = bload4(ra, off);
      araw[i][1] = bload4(ra, aok[i] ? off + 16 : kOOB);
    }
    if (p.s1) {
      const f32x4* sp = reinterpret_cast<const f32x4*>(p.s1 + 32 * ks + 8 * qk);
      const f32x4* tp = reinterpret_cast<const f32x4*>(p.t1 + 32 * ks + 8 * qk);
      sraw[0] = sp[0], sraw[1] = sp[1];
      traw[0] = tp[0], traw[1] = tp[1];
    }
#pragma unroll
    for (int pl = 0; pl < 2; ++pl)
#pragma unroll
      for (int c = 0; c < 2; ++c) braw[pl][c] = wsrc[(size_t)(ks * 2 + pl) * NT * 64 + tid + 256 * c];
  };
  bf16x8 ah[2], al[2];
  auto stage = [&](int buf) {
#pragma unroll
    for (int pl = 0; pl < 2; ++pl)
#pragma unroll
      for (int c = 0; c < 2; ++c)
        *reinterpret_cast<uint4*>(&smem[buf][(pl * 512 + tid + 256 * c) * 16]) = braw[pl][c];
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      float v[8];
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        const float a = araw[i][e >> 2][e & 3];
        v[e] = p.s1 ? fmaxf(fmaf(a, sraw[e >> 2][e & 3], traw[e >> 2][e & 3]), 0.f) : a;
      }
      split(v, ah[i], al[i]);
    }
  };

  f32x4 acc[2][8];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 8; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

  gload(0);
  stage(0);
  __syncthreads();
  for (int ks = 0; ks < KS; ++ks) {
    const bool more = ks + 1 < KS;
    if (more) gload(ks + 1);
    const unsigned char* w = smem[ks & 1];
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const bf16x8 bh = *reinterpret_cast<const bf16x8*>(w + (j * 64 + lane) * 16);
      const bf16x8 bl = *reinterpret_cast<const bf16x8*>(w + (512 + j * 64 + lane) * 16);
#pragma unroll
      for (int i = 0; i < 2; ++i) mma3(ah[i], al[i], bh, bl, acc[i][j]);
    }
    // the other buffer was last read in step ks - 1, which every wave left at the barrier below
    if (more) stage((ks + 1) & 1);
    __syncthreads();
  }

  // ---- epilogue: BN2 + ReLU (or none), store, segment column sums
  const __amdgpu_buffer_rsrc_t ro = make_rsrc(p.out);
  float csum[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    const int col = n0 + 16 * j + r16;
    const float sc = p.s2 ? p.s2[col] : 1.f, sh = p.s2 ? p.t2[col] : 0.f;
    float cs = 0.f;
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int lr = 32 * wave + 16 * i + 4 * qk + r;
        const bool ok = lr < nrows;
        float y = acc[i][j][r];
        if (p.s2) y = fmaxf(fmaf(y, sc, sh), 0.f);
        store1(ro, y, ok ? ((r0 + lr) * p.ldo + col) * 4 : kOOB);
        cs += ok ? y : 0.f;
      }
    csum[j] = cs;
  }
  if (p.segsum) {  // block-uniform
    float* red = reinterpret_cast<float*>(&smem[0][0]);  // [4 waves][128]; free after the loop's last barrier
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      float v = csum[j];
      v += __shfl_xor(v, 16, 64);
      v += __shfl_xor(v, 32, 64);
      if (qk == 0) red[wave * 128 + 16 * j + r16] = v;
    }
    __syncthreads();
    if (tid < 128) {
      const float v = ((red[tid] + red[128 + tid]) + red[256 + tid]) + red[384 + tid];
      p.segsum[(size_t)strip * p.N + n0 + tid] = v;
    }
  }
}

__global__ __launch_bounds__(256) void cam_bnrelu_kernel(const float* __restrict__ x, int ldx, int M, int K4,
                                                         const float* __restrict__ sc, const float* __restrict__ sh,
                                                         float* __restrict__ out, int ldo) {
  const long long n = (long long)M * K4;
  for (long long q = blockIdx.x * 256LL + threadIdx.x; q < n; q += (long long)gridDim.x * 256) {
    const int m = (int)(q / K4), c = (int)(q - (long long)m * K4) * 4;
    const f32x4 v = *reinterpret_cast<const f32x4*>(x + (size_t)m * ldx + c);
    const f32x4 a = *reinterpret_cast<const f32x4*>(sc + c);
    const f32x4 b = *reinterpret_cast<const f32x4*>(sh + c);
    f32x4 y;
#pragma unroll
    for (int e = 0; e < 4; ++e) y[e] = fmaxf(fmaf(v[e], a[e], b[e]), 0.f);
    *reinterpret_cast<f32x4*>(out + (size_t)m * ldo + c) = y;
  }
}

// ---------------------------------------------------------------------- context mask --
// One block of 64 threads per (utterance, segment).
__global__ __launch_bounds__(64) void cam_mask_kernel(const float* __restrict__ segsum, int T, int nseg,
                                                      const float* __restrict__ w1t, const float* __restrict__ b1,
                                                      const float* __restrict__ w2t, const float* __restrict__ b2,
                                                      float* __restrict__ mask) {
  __shared__ float ctx[128], hid[64];
  const int tid = threadIdx.x;
  const int b = blockIdx.x / nseg, sg = blockIdx.x - b * nseg;
  const int len = min(kCamSeg, T - sg * kCamSeg);
#pragma unroll
  for (int h = 0; h < 2; ++h) {
    const int c = tid + 64 * h;
    double tot = 0.0;
    for (int q = 0; q < nseg; ++q) tot += (double)segsum[((size_t)b * nseg + q) * 128 + c];
    const float mean_all = (float)(tot / (double)T);
    const float mean_seg = (float)((double)segsum[((size_t)b * nseg + sg) * 128 + c] / (double)len);
    ctx[c] = mean_all + mean_seg;
  }
  __syncthreads();
  float a = b1[tid];
  for (int k = 0; k < 128; ++k) a = fmaf(ctx[k], w1t[k * 64 + tid], a);
  hid[tid] = fmaxf(a, 0.f);
  __syncthreads();
  if (tid < 32) {
    float z = b2[tid];
    for (int k = 0; k < 64; ++k) z = fmaf(hid[k], w2t[k * 32 + tid], z);
    mask[(size_t)blockIdx.x * 32 + tid] = 1.f / (1.f + expf(-z));
  }
}

// ------------------------------------------------------------- masked local conv (k3) --
// One block = 128 rows, 4 waves of 32 rows x 32 columns; K = 3 taps x 128 channels = 12 k-steps,
// each inside one tap.  A and the W fragments (48 KB in all, cache resident) come straight
// from global memory.
__global__ __launch_bounds__(256) void cam_local_kernel(const CamLocalArgs p) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int r16 = lane & 15, qk = lane >> 4;
  const int m0 = blockIdx.x * 128 + 32 * wave;
  const int nseg = (p.T + kCamSeg - 1) / kCamSeg;
  const __amdgpu_buffer_rsrc_t rh = make_rsrc(p.h);
  int am[2], at[2];
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    const int m = m0 + 16 * i + r16;
    am[i] = m;
    at[i] = m < p.M ? m % p.T : -0x40000000;
  }
  const uint4* wsrc = reinterpret_cast<const uint4*>(p.w);
  f32x4 acc[2][2];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int ks = 0; ks < 12; ++ks) {
    const int d = ((ks >> 2) - 1) * p.dil, c0 = (ks & 3) * 32 + 8 * qk;
    bf16x8 ah[2], al[2];
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const int tt = at[i] + d;
      const bool ok = tt >= 0 && tt < p.T;
      const int off = ok ? ((am[i] + d) * p.ldh + c0) * 4 : kOOB;
      const f32x4 v0 = bload4(rh, off), v1 = bload4(rh, ok ? off + 16 : kOOB);
      const float v[8] = {v0[0], v0[1], v0[2], v0[3], v1[0], v1[1], v1[2], v1[3]};
      split(v, ah[i], al[i]);
    }
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const bf16x8 bh = __builtin_bit_cast(bf16x8, wsrc[((ks * 2 + 0) * 2 + j) * 64 + lane]);
      const bf16x8 bl = __builtin_bit_cast(bf16x8, wsrc[((ks * 2 + 1) * 2 + j) * 64 + lane]);
#pragma unroll
      for (int i = 0; i < 2; ++i) mma3(ah[i], al[i], bh, bl, acc[i][j]);
    }
  }
  const __amdgpu_buffer_rsrc_t ro = make_rsrc(p.out);
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int m = m0 + 16 * i + 4 * qk + r;
      const bool ok = m < p.M;
      const int mm = ok ? m : 0;
      const int b = mm / p.T, t = mm - b * p.T;
      const float* mk = p.mask + ((size_t)b * nseg + t / kCamSeg) * 32;
#pragma unroll
      for (int j = 0; j < 2; ++j) {
        const int col = 16 * j + r16;
        store1(ro, acc[i][j][r] * mk[col], ok ? (m * p.ldo + col) * 4 : kOOB);
      }
    }
}

}  // namespace

void launch_cam_gemm(const CamGemmArgs& p, hipStream_t s) {
  WSP_CHECK(p.M > 0 && p.T > 0 && p.K >= 32 && p.K % 32 == 0 && p.N > 0 && p.N % kGemmCols == 0,
            "cam_gemm: K % 32 == 0 and N % 128 == 0");
  WSP_CHECK(p.lda >= p.K && p.lda % 4 == 0 && p.ldo >= p.N, "cam_gemm: bad strides");
  WSP_CHECK((reinterpret_cast<uintptr_t>(p.a) & 15) == 0 && (reinterpret_cast<uintptr_t>(p.w) & 15) == 0 &&
                (!p.s1 || ((reinterpret_cast<uintptr_t>(p.s1) | reinterpret_cast<uintptr_t>(p.t1)) & 15) == 0),
            "cam_gemm: operands must be 16-byte aligned");
  WSP_CHECK((p.s1 == nullptr) == (p.t1 == nullptr) && (p.s2 == nullptr) == (p.t2 == nullptr),
            "cam_gemm: scale and shift come in pairs");
  WSP_CHECK((long long)p.M * p.lda * 4 < (long long)kOOB && (long long)p.M * p.ldo * 4 < (long long)kOOB,
            "cam_gemm: operand exceeds 2 GiB (split the batch)");
  long long gx;
  if (p.segsum) {
    WSP_CHECK(p.N == kGemmCols && p.M % p.T == 0, "cam_gemm: segment sums need N == 128 and M == B * T");
    gx = (long long)(p.M / p.T) * ((p.T + kCamSeg - 1) / kCamSeg);
  } else {
    gx = (p.M + kGemmRows - 1) / kGemmRows;
  }
  WSP_CHECK(gx < (1LL << 31), "cam_gemm: grid too large");
  hipLaunchKernelGGL(cam_gemm_kernel, dim3((unsigned)gx, p.N / kGemmCols), dim3(256), 0, s, p);
  WSP_HIP(hipGetLastError());
}

void launch_cam_bnrelu(const float* x, int ldx, int M, int K, const float* sc, const float* sh, float* out, int ldo,
                       hipStream_t s) {
  WSP_CHECK(M > 0 && K > 0 && K % 4 == 0 && ldx >= K && ldo >= K && ldx % 4 == 0 && ldo % 4 == 0,
            "cam_bnrelu: K, ldx, ldo multiples of 4");
  const long long n = (long long)M * (K / 4);
  const unsigned blocks = (unsigned)std::min<long long>((n + 255) / 256, 65536);
  hipLaunchKernelGGL(cam_bnrelu_kernel, dim3(blocks), dim3(256), 0, s, x, ldx, M, K / 4, sc, sh, out, ldo);
  WSP_HIP(hipGetLastError());
}

void launch_cam_mask(const float* segsum, int B, int T, const float* w1t, const float* b1, const float* w2t,
                     const float* b2, float* mask, hipStream_t s) {
  WSP_CHECK(B > 0 && T > 0, "cam_mask: empty batch");
  const int nseg = (T + kCamSeg - 1) / kCamSeg;
  WSP_CHECK((long long)B * nseg < (1LL << 31), "cam_mask: grid too large");
  hipLaunchKernelGGL(cam_mask_kernel, dim3((unsigned)(B * nseg)), dim3(64), 0, s, segsum, T, nseg, w1t, b1, w2t, b2,
                     mask);
  WSP_HIP(hipGetLastError());
}

void launch_cam_local(const CamLocalArgs& p, hipStream_t s) {
  WSP_CHECK(p.M > 0 && p.T > 0 && p.M % p.T == 0 && p.dil >= 1, "cam_local: M == B * T, dil >= 1");
  WSP_CHECK(p.ldh >= 128 && p.ldh % 4 == 0 && p.ldo >= 32, "cam_local: bad strides");
  WSP_CHECK((reinterpret_cast<uintptr_t>(p.h) & 15) == 0 && (reinterpret_cast<uintptr_t>(p.w) & 15) == 0,
            "cam_local: operands must be 16-byte aligned");
  WSP_CHECK((long long)p.M * p.ldh * 4 < (long long)kOOB && (long long)p.M * p.ldo * 4 < (long long)kOOB,
            "cam_local: operand exceeds 2 GiB (split the batch)");
  hipLaunchKernelGGL(cam_local_kernel, dim3((unsigned)((p.M + 127) / 128)), dim3(256), 0, s, p);
  WSP_HIP(hipGetLastError());
}

}  // namespace wsp
