// ERes2Net kernels (eres2net.py:75-240; eres2net.h has the contracts).
//
// The Res2 chain of an ERes2Net block works on channel slices 16 to 256 wide of NHWC tensors, and
// from stage 3 on every step first passes the AFF gate.  Both kernels here run their MFMAs with the
// weights as the A operand and 16 positions as the B operand's columns:
//
//   v_mfma_f32_16x16x32_bf16: lane l holds A[row l & 15][k = 8 (l >> 4) .. + 7] and
//   B[k = 8 (l >> 4) .. + 7][column l & 15]; accumulator register r is row 4 (l >> 4) + r,
//   column l & 15.
//
// so a lane ends up with four consecutive output channels of one position.  eres_conv_kernel is
// the implicit GEMM over taps x cin (the 3x3 Res2 step and, with one tap, the 1x1 convs with their
// 2-D stride gather, residual and clamp); weight fragments come straight from global memory (they
// are at most a few hundred KB and stay in L2); with EresConvArgs::ksplit the 1x1 conv reads a
// concatenated operand, channels below ksplit from a and the rest from a2 (Res2Net's conv3: a k-step
// lies in one source where ksplit % 32 == 0, else a lane loads from both, one of them out of range).
// eres_aff_kernel keeps the AFF's hidden row
// (C / 4 channels) in accumulators: two stacked 16-channel tiles are exactly one 32-long k-step
// of the second product's B operand, in the k order pack::frag16(acc_order) gives its weights.
#include "eres2net.h"

#include "bf16x3.h"
#include "gemm_common.h"

namespace wsp {

namespace {

__device__ __forceinline__ void store4(__amdgpu_buffer_rsrc_t r, const f32x4 y, int off) {
  __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4, y), r, off, 0, 0);
}

__device__ __forceinline__ void split8(const f32x4 v0, const f32x4 v1, bf16x8& hi, bf16x8& lo) {
  const float v[8] = {v0[0], v0[1], v0[2], v0[3], v1[0], v1[1], v1[2], v1[3]};
  split(v, hi, lo);
}

// ------------------------------------------------------------------ conv (3x3 / 1x1) --
struct ConvGeom {
  int Fo, To, M, K, KS, tiles, taps, pad;
};

// One block = 4 waves; a wave owns PT x 16 positions and NT x 16 output channels.  TAPS = 9: the
// activations are loaded one k-step ahead (9 c / 32 steps of MFMAs to hide them under); TAPS = 1
// loads them where they are used: the 1x1 convs are short (K = 32 .. 576) and HBM-bound in the
// early stages, where the registers of a second set cost more in occupancy than they hide.
template <int NT, int PT, int TAPS>
__global__ __launch_bounds__(256) void eres_conv_kernel(const EresConvArgs p, const ConvGeom g) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int r16 = lane & 15, qk = lane >> 4;
  const int m0 = (blockIdx.x * 4 + wave) * (16 * PT);
  if (m0 >= g.M) return;  // wave-uniform; the kernel has no barrier
  const int jt0 = blockIdx.y * NT;
  const __amdgpu_buffer_rsrc_t ra = make_rsrc(p.a);
  const __amdgpu_buffer_rsrc_t ra2 = make_rsrc(p.a2 ? p.a2 : p.a);
  int ib[PT], fi0[PT], ti0[PT];
  bool live[PT];
#pragma unroll
  for (int pt = 0; pt < PT; ++pt) {
    const int m = m0 + 16 * pt + r16;
    live[pt] = m < g.M;
    const int mm = live[pt] ? m : 0;
    const int b = mm / (g.Fo * g.To), rem = mm - b * g.Fo * g.To;
    const int fo = rem / g.To, to = rem - fo * g.To;
    fi0[pt] = fo * p.stride - g.pad;
    ti0[pt] = to * p.stride - g.pad;
    ib[pt] = b * p.Fi * p.Ti;
  }
  const uint4* wsrc = reinterpret_cast<const uint4*>(p.w);
  f32x4 acc[PT][NT];
#pragma unroll
  for (int pt = 0; pt < PT; ++pt)
#pragma unroll
    for (int j = 0; j < NT; ++j) acc[pt][j] = f32x4{0.f, 0.f, 0.f, 0.f};

  // the activations of k-step ks, raw: v = a, u = a2 (zero without one)
  auto gload = [&](int ks, f32x4 (&v)[PT][2], f32x4 (&u)[PT][2]) {
    // a lane's 8 consecutive k stay inside one tap (cin % 8 == 0)
    const int k8 = 32 * ks + 8 * qk;
    const bool kin = k8 < g.K;
    const int tap = k8 / p.cin, c = k8 - tap * p.cin;
    const int kf = TAPS == 9 ? tap / 3 : 0, kt = tap - 3 * kf;
#pragma unroll
    for (int pt = 0; pt < PT; ++pt) {
      const int fi = fi0[pt] + kf, ti = ti0[pt] + kt;
      const bool ok = live[pt] && kin && fi >= 0 && fi < p.Fi && ti >= 0 && ti < p.Ti;
      const int row = ok ? ib[pt] + fi * p.Ti + ti : 0;
      if (TAPS == 1 && p.ksplit > 0 && (p.ksplit & 31) == 0) {  // concatenated operand, a k-step in one source
        if (32 * ks < p.ksplit) {                                 // (wave-uniform)
          const int off = ok ? (row * p.lda + c) * 4 : kOOB;
          v[pt][0] = bload4(ra, off);
          v[pt][1] = bload4(ra, ok ? off + 16 : kOOB);
        } else {
          const int off = ok ? (row * p.lda2 + c - p.ksplit) * 4 : kOOB;
          v[pt][0] = bload4(ra2, off);
          v[pt][1] = bload4(ra2, ok ? off + 16 : kOOB);
        }
        continue;
      }
      if (TAPS == 1 && p.ksplit > 0) {  // the split inside a k-step: both loads, one of them out of range (zeros)
        const bool lo = c < p.ksplit;
        const int off = ok && lo ? (row * p.lda + c) * 4 : kOOB;
        const int off2 = ok && !lo ? (row * p.lda2 + c - p.ksplit) * 4 : kOOB;
        v[pt][0] = bload4(ra, off) + bload4(ra2, off2);
        v[pt][1] = bload4(ra, ok && lo ? off + 16 : kOOB) + bload4(ra2, ok && !lo ? off2 + 16 : kOOB);
        continue;
      }
      const int off = ok ? (row * p.lda + c) * 4 : kOOB;
      v[pt][0] = bload4(ra, off);
      v[pt][1] = bload4(ra, ok ? off + 16 : kOOB);
      if (TAPS == 9 && p.a2) {  // only the Res2 step takes an added slice
        const int off2 = ok ? (row * p.lda2 + c) * 4 : kOOB;
        u[pt][0] = bload4(ra2, off2);
        u[pt][1] = bload4(ra2, ok ? off2 + 16 : kOOB);
      }
    }
  };
  f32x4 v[PT][2], u[PT][2];
#pragma unroll
  for (int pt = 0; pt < PT; ++pt) u[pt][0] = u[pt][1] = f32x4{0.f, 0.f, 0.f, 0.f};
  if constexpr (TAPS == 9) gload(0, v, u);
  for (int ks = 0; ks < g.KS; ++ks) {
    if constexpr (TAPS == 1) gload(ks, v, u);
    bf16x8 bh[PT], bl[PT];
#pragma unroll
    for (int pt = 0; pt < PT; ++pt) {
      if constexpr (TAPS == 9)  // the Res2 chain's sp + spx[i], summed in f32 before the split
        split8(v[pt][0] + u[pt][0], v[pt][1] + u[pt][1], bh[pt], bl[pt]);
      else
        split8(v[pt][0], v[pt][1], bh[pt], bl[pt]);
    }
    if constexpr (TAPS == 9)  // one k-step ahead: in flight under this step's MFMAs
      if (ks + 1 < g.KS) gload(ks + 1, v, u);
#pragma unroll
    for (int j = 0; j < NT; ++j) {
      if (jt0 + j >= g.tiles) continue;  // wave-uniform
      const bf16x8 wh = __builtin_bit_cast(bf16x8, wsrc[((size_t)(ks * 2 + 0) * g.tiles + jt0 + j) * 64 + lane]);
      const bf16x8 wl = __builtin_bit_cast(bf16x8, wsrc[((size_t)(ks * 2 + 1) * g.tiles + jt0 + j) * 64 + lane]);
#pragma unroll
      for (int pt = 0; pt < PT; ++pt) mma3(wh, wl, bh[pt], bl[pt], acc[pt][j]);
    }
  }

  // ---- epilogue: bias (+ residual), activation, 16-byte stores of 4 channels
  const __amdgpu_buffer_rsrc_t ro = make_rsrc(p.out);
  const __amdgpu_buffer_rsrc_t rb = make_rsrc(p.bias);
  const __amdgpu_buffer_rsrc_t rr = make_rsrc(p.res ? p.res : p.bias);
#pragma unroll
  for (int j = 0; j < NT; ++j) {
    const int c = (jt0 + j) * 16 + 4 * qk;
    const bool cok = c < p.N;  // N % 4 == 0: the four channels are in or out together
    const f32x4 bv = bload4(rb, cok ? c * 4 : kOOB);
#pragma unroll
    for (int pt = 0; pt < PT; ++pt) {
      const int m = m0 + 16 * pt + r16;
      const bool ok = cok && m < g.M;
      f32x4 y = acc[pt][j] + bv;
      if (p.res) y += bload4(rr, ok ? (m * p.ldres + c) * 4 : kOOB);
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        if (p.act != kEresNone) y[e] = fmaxf(y[e], 0.f);
        if (p.act == kEresClamp) y[e] = fminf(y[e], 20.f);
      }
      store4(ro, y, ok ? (m * p.ldo + c) * 4 : kOOB);
    }
  }
}

// ------------------------------------------------------------------------------- AFF --
// One block = 4 waves; a wave owns PT x 16 positions and the whole hidden row (HT x 16 channels).
template <int HT, int PT>
__global__ __launch_bounds__(256) void eres_aff_kernel(const EresAffArgs p) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int r16 = lane & 15, qk = lane >> 4;
  const int m0 = (blockIdx.x * 4 + wave) * (16 * PT);
  if (m0 >= p.M) return;  // wave-uniform; the kernel has no barrier
  const __amdgpu_buffer_rsrc_t rx = make_rsrc(p.x);
  const __amdgpu_buffer_rsrc_t ry = make_rsrc(p.y);
  int offx[PT], offy[PT];
  bool live[PT];
#pragma unroll
  for (int pt = 0; pt < PT; ++pt) {
    const int m = m0 + 16 * pt + r16;
    live[pt] = m < p.M;
    offx[pt] = live[pt] ? (m * p.ldx + 8 * qk) * 4 : 0;
    offy[pt] = live[pt] ? (m * p.ldy + 8 * qk) * 4 : 0;
  }
  // ---- h^T = Wa [x | y]^T: k-steps [0, C / 32) read x, the rest y
  const uint4* wa = reinterpret_cast<const uint4*>(p.wa);
  f32x4 acc[PT][HT];
#pragma unroll
  for (int pt = 0; pt < PT; ++pt)
#pragma unroll
    for (int t = 0; t < HT; ++t) acc[pt][t] = f32x4{0.f, 0.f, 0.f, 0.f};
  const int KSx = p.C / 32;
  for (int ks = 0; ks < 2 * KSx; ++ks) {
    const bool isx = ks < KSx;
    const int kc = (isx ? ks : ks - KSx) * 128;
    bf16x8 bh[PT], bl[PT];
#pragma unroll
    for (int pt = 0; pt < PT; ++pt) {
      f32x4 v0, v1;
      if (isx) {
        const int off = live[pt] ? offx[pt] + kc : kOOB;
        v0 = bload4(rx, off), v1 = bload4(rx, live[pt] ? off + 16 : kOOB);
      } else {
        const int off = live[pt] ? offy[pt] + kc : kOOB;
        v0 = bload4(ry, off), v1 = bload4(ry, live[pt] ? off + 16 : kOOB);
      }
      split8(v0, v1, bh[pt], bl[pt]);
    }
#pragma unroll
    for (int t = 0; t < HT; ++t) {
      const bf16x8 wh = __builtin_bit_cast(bf16x8, wa[((size_t)(ks * 2 + 0) * HT + t) * 64 + lane]);
      const bf16x8 wl = __builtin_bit_cast(bf16x8, wa[((size_t)(ks * 2 + 1) * HT + t) * 64 + lane]);
#pragma unroll
      for (int pt = 0; pt < PT; ++pt) mma3(wh, wl, bh[pt], bl[pt], acc[pt][t]);
    }
  }
  // ---- bias + SiLU; tiles 2 s and 2 s + 1 are k-step s of the second product's B operand:
  // element e of lane group qk is hidden channel 32 s + 16 (e >> 2) + 4 qk + (e & 3)
  bf16x8 hh[PT][HT / 2], hl[PT][HT / 2];
#pragma unroll
  for (int s2 = 0; s2 < HT / 2; ++s2) {
    const f32x4 b0 = *reinterpret_cast<const f32x4*>(p.ba + 32 * s2 + 4 * qk);
    const f32x4 b1 = *reinterpret_cast<const f32x4*>(p.ba + 32 * s2 + 16 + 4 * qk);
#pragma unroll
    for (int pt = 0; pt < PT; ++pt) {
      float v[8];
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const float u0 = acc[pt][2 * s2][r] + b0[r], u1 = acc[pt][2 * s2 + 1][r] + b1[r];
        v[r] = u0 / (1.f + expf(-u0));
        v[4 + r] = u1 / (1.f + expf(-u1));
      }
      split(v, hh[pt][s2], hl[pt][s2]);
    }
  }
  // ---- g = 1 + tanh(Wb h + bb), out = x g + y (2 - g), 16 channels at a time
  const uint4* wb = reinterpret_cast<const uint4*>(p.wb);
  const __amdgpu_buffer_rsrc_t ro = make_rsrc(p.out);
  const int CT = p.C / 16;
  for (int ct = 0; ct < CT; ++ct) {
    f32x4 z[PT];
#pragma unroll
    for (int pt = 0; pt < PT; ++pt) z[pt] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int s2 = 0; s2 < HT / 2; ++s2) {
      const bf16x8 wh = __builtin_bit_cast(bf16x8, wb[((size_t)(s2 * 2 + 0) * CT + ct) * 64 + lane]);
      const bf16x8 wl = __builtin_bit_cast(bf16x8, wb[((size_t)(s2 * 2 + 1) * CT + ct) * 64 + lane]);
#pragma unroll
      for (int pt = 0; pt < PT; ++pt) mma3(wh, wl, hh[pt][s2], hl[pt][s2], z[pt]);
    }
    const int c = 16 * ct + 4 * qk;
    const f32x4 bv = *reinterpret_cast<const f32x4*>(p.bb + c);
#pragma unroll
    for (int pt = 0; pt < PT; ++pt) {
      const int m = m0 + 16 * pt + r16;
      const bool ok = m < p.M;
      const f32x4 xv = bload4(rx, ok ? (m * p.ldx + c) * 4 : kOOB);
      const f32x4 yv = bload4(ry, ok ? (m * p.ldy + c) * 4 : kOOB);
      f32x4 o;
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const float gt = 1.f + tanhf(z[pt][e] + bv[e]);
        o[e] = xv[e] * gt + yv[e] * (2.f - gt);
      }
      store4(ro, o, ok ? (m * p.ldo + c) * 4 : kOOB);
    }
  }
}

bool aligned16(const void* q) { return (reinterpret_cast<uintptr_t>(q) & 15) == 0; }

template <int NT>
void launch_conv_nt(const EresConvArgs& p, const ConvGeom& g, hipStream_t s) {
  constexpr int PT = 2;
  const long long gx = ((long long)g.M + 64 * PT - 1) / (64 * PT);
  WSP_CHECK(gx < (1LL << 31), "eres_conv: grid too large");
  const dim3 grid((unsigned)gx, (g.tiles + NT - 1) / NT);
  if (g.taps == 9)
    hipLaunchKernelGGL((eres_conv_kernel<NT, PT, 9>), grid, dim3(256), 0, s, p, g);
  else
    hipLaunchKernelGGL((eres_conv_kernel<NT, PT, 1>), grid, dim3(256), 0, s, p, g);
  WSP_HIP(hipGetLastError());
}

void launch_conv(const EresConvArgs& p, int taps, hipStream_t s) {
  WSP_CHECK(p.B > 0 && p.Fi > 0 && p.Ti > 0 && p.cin > 0 && p.N > 0 && (p.stride == 1 || p.stride == 2),
            "eres_conv: bad shape");
  WSP_CHECK(p.cin % 8 == 0 && p.N % 4 == 0, "eres_conv: cin % 8 == 0 and N % 4 == 0");
  WSP_CHECK(p.lda >= (p.ksplit > 0 ? 8 : p.cin) && p.lda % 4 == 0 && p.ldo >= p.N && p.ldo % 4 == 0, "eres_conv: bad strides");
  WSP_CHECK(p.ksplit == 0 || taps == 1, "eres_conv: ksplit goes with the 1x1 conv only");
  WSP_CHECK(p.ksplit == 0 || (p.ksplit > 0 && p.ksplit % 8 == 0 && p.ksplit < p.cin),
            "eres_conv: ksplit must be a multiple of 8 below cin");
  WSP_CHECK(p.ksplit == 0 || p.a2, "eres_conv: ksplit needs the second operand a2");
  WSP_CHECK(!p.a2 || (p.lda2 >= (p.ksplit ? p.cin - p.ksplit : p.cin) && p.lda2 % 4 == 0),
            "eres_conv: bad stride of the added slice");
  WSP_CHECK(p.ksplit == 0 || p.lda >= p.ksplit, "eres_conv: bad strides");
  WSP_CHECK(!p.res || (p.ldres >= p.N && p.ldres % 4 == 0), "eres_conv: bad residual stride");
  WSP_CHECK(aligned16(p.a) && aligned16(p.a2) && aligned16(p.w) && aligned16(p.bias) && aligned16(p.res) &&
                aligned16(p.out) && p.bias && p.w && p.a && p.out,
            "eres_conv: operands must be 16-byte aligned");
  WSP_CHECK(p.act >= kEresNone && p.act <= kEresClamp, "eres_conv: bad activation");
  ConvGeom g;
  g.taps = taps;
  g.pad = taps == 9 ? 1 : 0;
  g.Fo = (p.Fi - 1) / p.stride + 1;
  g.To = (p.Ti - 1) / p.stride + 1;
  const long long M = (long long)p.B * g.Fo * g.To, in_rows = (long long)p.B * p.Fi * p.Ti;
  WSP_CHECK(in_rows * p.lda * 4 < (long long)kOOB && (!p.a2 || in_rows * p.lda2 * 4 < (long long)kOOB) &&
                M * p.ldo * 4 < (long long)kOOB && (!p.res || M * p.ldres * 4 < (long long)kOOB),
            "eres_conv: operand exceeds 2 GiB (split the batch)");
  g.M = (int)M;
  g.K = taps * p.cin;
  g.KS = (g.K + 31) / 32;
  g.tiles = (p.N + 15) / 16;
  // channel tiles per wave: as many as there are (up to 8: the activations are read once per
  // 128 channels), fewer while the grid would leave CUs without two blocks.  Every output's
  // k order is the same whatever the split, so the result does not depend on it
  int nt = g.tiles >= 8 ? 8 : g.tiles >= 4 ? 4 : g.tiles >= 2 ? 2 : 1;
  const long long row_blocks = (M + 127) / 128, want = 2LL * device_cu_count();
  while (nt > 1 && row_blocks * ((g.tiles + nt - 1) / nt) < want) nt /= 2;
  if (nt == 8)
    launch_conv_nt<8>(p, g, s);
  else if (nt == 4)
    launch_conv_nt<4>(p, g, s);
  else if (nt == 2)
    launch_conv_nt<2>(p, g, s);
  else
    launch_conv_nt<1>(p, g, s);
}

template <int HT, int PT>
void launch_aff_ht(const EresAffArgs& p, hipStream_t s) {
  const long long gx = ((long long)p.M + 64 * PT - 1) / (64 * PT);
  WSP_CHECK(gx < (1LL << 31), "eres_aff: grid too large");
  hipLaunchKernelGGL((eres_aff_kernel<HT, PT>), dim3((unsigned)gx), dim3(256), 0, s, p);
  WSP_HIP(hipGetLastError());
}

}  // namespace

bool eres_conv3x3_supported(int w) {
  for (int k : {16, 24, 32, 48, 64, 96, 128, 192, 256})
    if (w == k) return true;
  return false;
}

void launch_eres_conv3x3(const EresConvArgs& p, hipStream_t s) {
  WSP_CHECK(p.ksplit == 0, "eres_conv3x3: ksplit goes with the 1x1 conv only");
  WSP_CHECK(eres_conv3x3_supported(p.cin) && p.N == p.cin && p.stride == 1,
            "eres_conv3x3: stride 1, width in {16, 24, 32, 48, 64, 96, 128, 192, 256}");
  launch_conv(p, 9, s);
}

void launch_eres_pw(const EresConvArgs& p, hipStream_t s) {
  WSP_CHECK(!p.a2 || p.ksplit != 0, "eres_pw: no added slice");
  launch_conv(p, 1, s);
}

bool eres_aff_supported(int C) {
  for (int k : {64, 96, 128, 192, 256, 512, 1024, 2048})
    if (C == k) return true;
  return false;
}

void launch_eres_aff(const EresAffArgs& p, hipStream_t s) {
  WSP_CHECK(p.M > 0 && eres_aff_supported(p.C), "eres_aff: C in {64, 96, 128, 192, 256, 512, 1024, 2048}");
  WSP_CHECK(p.ldx >= p.C && p.ldy >= p.C && p.ldo >= p.C && p.ldx % 4 == 0 && p.ldy % 4 == 0 && p.ldo % 4 == 0,
            "eres_aff: bad strides");
  WSP_CHECK(p.x && p.y && p.out && p.wa && p.wb && p.ba && p.bb && aligned16(p.x) && aligned16(p.y) &&
                aligned16(p.out) && aligned16(p.wa) && aligned16(p.wb) && aligned16(p.ba) && aligned16(p.bb),
            "eres_aff: operands must be 16-byte aligned");
  WSP_CHECK((long long)p.M * p.ldx * 4 < (long long)kOOB && (long long)p.M * p.ldy * 4 < (long long)kOOB &&
                (long long)p.M * p.ldo * 4 < (long long)kOOB,
            "eres_aff: operand exceeds 2 GiB (split the batch)");
  const int Hp = (p.C / 4 + 31) / 32 * 32;
  // 16 positions per wave instead of 64 / 32 while the grid would leave CUs without two blocks
  // (a position's arithmetic is the same either way)
  const bool few = ((long long)p.M + 255) / 256 < 2LL * device_cu_count();
  switch (Hp / 16) {
    case 2: return few ? launch_aff_ht<2, 1>(p, s) : launch_aff_ht<2, 4>(p, s);
    case 4: return few ? launch_aff_ht<4, 1>(p, s) : launch_aff_ht<4, 4>(p, s);
    case 8: return few ? launch_aff_ht<8, 1>(p, s) : launch_aff_ht<8, 4>(p, s);
    case 16: return few ? launch_aff_ht<16, 1>(p, s) : launch_aff_ht<16, 2>(p, s);
    case 32: return launch_aff_ht<32, 1>(p, s);
    default: WSP_CHECK(false, "eres_aff: unsupported hidden width");
  }
}

}  // namespace wsp
