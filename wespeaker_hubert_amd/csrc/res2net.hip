// Res2Net block tail (res2net.py:66-93; res2net.h has the contract): the 3x3 conv over the first
// channel slice of the block's conv1 output, the concatenation with the bypassed second slice and
// conv3 + residual + clamp, one launch.
//
// The MFMAs run transposed as in eres2net.hip (v_mfma_f32_16x16x32_bf16, weights = A operand, 16
// positions = B columns; accumulator register r of lane l is channel 4 (l >> 4) + r of position
// l & 15).  A wave owns PT x 16 positions and ALL w channels of s: the 3x3 conv is the implicit GEMM
// of eres_conv_kernel over 9 w / 32 k-steps (activations one k-step ahead, weight fragments from L2),
// into WT = w / 16 accumulator tiles.  Bias and clamp are applied in f32 on the accumulators; two
// stacked tiles are then exactly one 32-long k-step of conv3's B operand in the k order
// pack::frag16(acc_order) gives W3 (eres_aff_kernel's mechanism), so s is split to bf16 hi / lo
// where it stands and never goes to LDS or memory.  The bypassed slice y[:, w:] is conv3's k-steps
// WT / 2 .. WT - 1 in the same order (two 16-byte loads per lane and k-step: channels
// 32 s + 4 (l >> 4) .. + 3 and + 16); at w = 16 tile 0 of s and y[:, 16:] share k-step 0.  conv3 then
// runs 16 output channels at a time: WT k-steps of mma3 into one accumulator per position tile,
// bias + residual + clamp, 16-byte stores.  No barrier, no LDS: waves are independent, so there is
// no exchange between the four waves of a block and a position's arithmetic does not depend on the
// grid.
//
// Budget at w = 256 (WT = 16, PT = 1), VGPRs per lane: sixteen 3x3 accumulator tiles 64; they die as
// they are converted into the eight hi / lo k-steps of s, 8 x 2 x 4 = 64; the eight hi / lo k-steps
// of the bypassed slice another 64; the 3x3 loop's two raw activation sets 16, its hi / lo 8 and one
// weight fragment pair 8; conv3's accumulator 4 and its fragment pairs in flight 16.  hipcc allocates
// 164 VGPRs + 64 AGPRs, no spill, of the 512 a wave has at one wave per SIMD (256 threads per
// block).  LDS: 0 bytes.  Widths 16 .. 128 take PT = 2 (WT = 8: 64 accumulator registers and 2 x 64
// of operands per position tile; 156 VGPRs + 64 AGPRs).
#include "res2net.h"

#include "bf16x3.h"
#include "gemm_common.h"

namespace wsp {

namespace {

struct TailGeom {
  int M, K, KS, tiles;
};

template <int WT, int PT>
__global__ __launch_bounds__(256) void res2_tail_kernel(const Res2TailArgs p, const TailGeom g) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int r16 = lane & 15, qk = lane >> 4;
  const int m0 = (blockIdx.x * 4 + wave) * (16 * PT);
  if (m0 >= g.M) return;  // wave-uniform; the kernel has no barrier
  const __amdgpu_buffer_rsrc_t ry = make_rsrc(p.y);
  int ib[PT], f0[PT], t0[PT];
  bool live[PT];
#pragma unroll
  for (int pt = 0; pt < PT; ++pt) {
    const int m = m0 + 16 * pt + r16;
    live[pt] = m < g.M;
    const int mm = live[pt] ? m : 0;
    const int b = mm / (p.F * p.T), rem = mm - b * p.F * p.T;
    const int f = rem / p.T;
    f0[pt] = f - 1;
    t0[pt] = rem - f * p.T - 1;
    ib[pt] = b * p.F * p.T;
  }

  // ---- s^T = W1 im2col(y[:, :w])^T: eres_conv_kernel's 3x3 loop with every channel tile in this wave
  const uint4* w1 = reinterpret_cast<const uint4*>(p.w1);
  f32x4 acc[PT][WT];
#pragma unroll
  for (int pt = 0; pt < PT; ++pt)
#pragma unroll
    for (int j = 0; j < WT; ++j) acc[pt][j] = f32x4{0.f, 0.f, 0.f, 0.f};
  auto gload = [&](int ks, f32x4 (&v)[PT][2]) {
    // a lane's 8 consecutive k stay inside one tap (w % 8 == 0)
    const int k8 = 32 * ks + 8 * qk;
    const bool kin = k8 < g.K;
    const int tap = k8 / p.w, c = k8 - tap * p.w;
    const int kf = tap / 3, kt = tap - 3 * kf;
#pragma unroll
    for (int pt = 0; pt < PT; ++pt) {
      const int fi = f0[pt] + kf, ti = t0[pt] + kt;
      const bool ok = live[pt] && kin && fi >= 0 && fi < p.F && ti >= 0 && ti < p.T;
      const int off = ok ? ((ib[pt] + fi * p.T + ti) * p.ldy + c) * 4 : kOOB;
      v[pt][0] = bload4(ry, off);
      v[pt][1] = bload4(ry, ok ? off + 16 : kOOB);
    }
  };
  f32x4 v[PT][2];
  gload(0, v);
  for (int ks = 0; ks < g.KS; ++ks) {
    bf16x8 bh[PT], bl[PT];
#pragma unroll
    for (int pt = 0; pt < PT; ++pt) {
      const float x[8] = {v[pt][0][0], v[pt][0][1], v[pt][0][2], v[pt][0][3],
                          v[pt][1][0], v[pt][1][1], v[pt][1][2], v[pt][1][3]};
      split(x, bh[pt], bl[pt]);
    }
    if (ks + 1 < g.KS) gload(ks + 1, v);  // one k-step ahead: in flight under this step's MFMAs
#pragma unroll
    for (int j = 0; j < WT; ++j) {
      const bf16x8 wh = __builtin_bit_cast(bf16x8, w1[((size_t)(ks * 2 + 0) * WT + j) * 64 + lane]);
      const bf16x8 wl = __builtin_bit_cast(bf16x8, w1[((size_t)(ks * 2 + 1) * WT + j) * 64 + lane]);
#pragma unroll
      for (int pt = 0; pt < PT; ++pt) mma3(wh, wl, bh[pt], bl[pt], acc[pt][j]);
    }
  }

  // ---- conv3's B operand [s | y[:, w:]], WT k-steps in acc order: element e of lane group qk of
  // k-step s2 is concatenated channel 32 s2 + 16 (e >> 2) + 4 qk + (e & 3).  Channels below w are s
  // (bias, clamp, then the split), the rest the same column of y
  bf16x8 ch[PT][WT], cl[PT][WT];
#pragma unroll
  for (int s2 = 0; s2 < WT; ++s2) {
#pragma unroll
    for (int pt = 0; pt < PT; ++pt) {
      float x[8];
#pragma unroll
      for (int half = 0; half < 2; ++half) {
        const int c = 32 * s2 + 16 * half + 4 * qk;  // wave-uniform side of the concatenation
        if (2 * s2 + half < WT) {
          const f32x4 bv = *reinterpret_cast<const f32x4*>(p.b1 + c);
#pragma unroll
          for (int r = 0; r < 4; ++r) x[4 * half + r] = fminf(fmaxf(acc[pt][2 * s2 + half][r] + bv[r], 0.f), 20.f);
        } else {
          const int m = m0 + 16 * pt + r16;
          const f32x4 yv = bload4(ry, live[pt] ? (m * p.ldy + c) * 4 : kOOB);
#pragma unroll
          for (int r = 0; r < 4; ++r) x[4 * half + r] = yv[r];
        }
      }
      split(x, ch[pt][s2], cl[pt][s2]);
    }
  }

  // ---- out = clamp(b3 + W3 [s | y2] + res), 16 channels at a time
  const uint4* w3 = reinterpret_cast<const uint4*>(p.w3);
  const __amdgpu_buffer_rsrc_t ro = make_rsrc(p.out);
  const __amdgpu_buffer_rsrc_t rb = make_rsrc(p.b3);
  const __amdgpu_buffer_rsrc_t rr = make_rsrc(p.res ? p.res : p.b3);
#pragma unroll 2
  for (int ct = 0; ct < g.tiles; ++ct) {
    f32x4 z[PT];
#pragma unroll
    for (int pt = 0; pt < PT; ++pt) z[pt] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int s2 = 0; s2 < WT; ++s2) {
      const bf16x8 wh = __builtin_bit_cast(bf16x8, w3[((size_t)(s2 * 2 + 0) * g.tiles + ct) * 64 + lane]);
      const bf16x8 wl = __builtin_bit_cast(bf16x8, w3[((size_t)(s2 * 2 + 1) * g.tiles + ct) * 64 + lane]);
#pragma unroll
      for (int pt = 0; pt < PT; ++pt) mma3(wh, wl, ch[pt][s2], cl[pt][s2], z[pt]);
    }
    const int c = 16 * ct + 4 * qk;
    const bool cok = c < p.N;  // N % 4 == 0: the four channels are in or out together
    const f32x4 bv = bload4(rb, cok ? c * 4 : kOOB);
#pragma unroll
    for (int pt = 0; pt < PT; ++pt) {
      const int m = m0 + 16 * pt + r16;
      const bool ok = cok && m < g.M;
      f32x4 o = z[pt] + bv;
      if (p.res) o += bload4(rr, ok ? (m * p.ldres + c) * 4 : kOOB);
#pragma unroll
      for (int e = 0; e < 4; ++e) o[e] = fminf(fmaxf(o[e], 0.f), 20.f);
      __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4, o), ro, ok ? (m * p.ldo + c) * 4 : kOOB, 0, 0);
    }
  }
}

bool aligned16(const void* q) { return (reinterpret_cast<uintptr_t>(q) & 15) == 0; }

template <int WT, int PT>
void launch_wt(const Res2TailArgs& p, const TailGeom& g, hipStream_t s) {
  const long long gx = ((long long)g.M + 64 * PT - 1) / (64 * PT);
  WSP_CHECK(gx < (1LL << 31), "res2_tail: grid too large");
  hipLaunchKernelGGL((res2_tail_kernel<WT, PT>), dim3((unsigned)gx), dim3(256), 0, s, p, g);
  WSP_HIP(hipGetLastError());
}

}  // namespace

bool res2_tail_supported(int w) {
  for (int k : {16, 32, 64, 128, 256})
    if (w == k) return true;
  return false;
}

void launch_res2_tail(const Res2TailArgs& p, hipStream_t s) {
  WSP_CHECK(res2_tail_supported(p.w), "res2_tail: width in {16, 32, 64, 128, 256}");
  WSP_CHECK(p.B > 0 && p.F > 0 && p.T > 0 && p.N > 0 && p.N % 4 == 0, "res2_tail: bad shape");
  WSP_CHECK(p.ldy >= 2 * p.w && p.ldy % 4 == 0 && p.ldo >= p.N && p.ldo % 4 == 0, "res2_tail: bad strides");
  WSP_CHECK(!p.res || (p.ldres >= p.N && p.ldres % 4 == 0), "res2_tail: bad residual stride");
  WSP_CHECK(p.y && p.w1 && p.b1 && p.w3 && p.b3 && p.out && aligned16(p.y) && aligned16(p.w1) && aligned16(p.b1) &&
                aligned16(p.w3) && aligned16(p.b3) && aligned16(p.res) && aligned16(p.out),
            "res2_tail: operands must be 16-byte aligned");
  const long long M = (long long)p.B * p.F * p.T;
  WSP_CHECK(M * p.ldy * 4 < (long long)kOOB && M * p.ldo * 4 < (long long)kOOB &&
                (!p.res || M * p.ldres * 4 < (long long)kOOB),
            "res2_tail: operand exceeds 2 GiB (split the batch)");
  TailGeom g;
  g.M = (int)M;
  g.K = 9 * p.w;
  g.KS = (g.K + 31) / 32;
  g.tiles = (p.N + 15) / 16;
  // 16 positions per wave instead of 32 while the grid would leave CUs without two blocks (a
  // position's arithmetic is the same either way)
  const bool few = (M + 127) / 128 < 2LL * device_cu_count();
  switch (p.w / 16) {
    case 1: return few ? launch_wt<1, 1>(p, g, s) : launch_wt<1, 2>(p, g, s);
    case 2: return few ? launch_wt<2, 1>(p, g, s) : launch_wt<2, 2>(p, g, s);
    case 4: return few ? launch_wt<4, 1>(p, g, s) : launch_wt<4, 2>(p, g, s);
    case 8: return few ? launch_wt<8, 1>(p, g, s) : launch_wt<8, 2>(p, g, s);
    default: return launch_wt<16, 1>(p, g, s);
  }
}

}  // namespace wsp
