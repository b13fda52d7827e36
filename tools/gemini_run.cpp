// Op-level runner for the Gemini DF-ResNet kernels (tests/test_gpu_gemini_op.py).
// Launches launch_gemini_dw, launch_gemini_tail, launch_gemini_down and, for the bottleneck's 1x1
// convs, launch_conv_gemm_x3 with the family's tile family 7 of libwsp_hip.so, with weights packed by
// the library's own pack::frag16 / pack::conv_kmajor / pack::split.  Framing, case and result files:
// tools/op_runner.h.  Magic 'WSPG' (0x47505357).  Arrays are f32; one result array per case.
//
//   op 1  depthwise 3x3     hdr = B, F, T, C, ldy, yoff, ldo, ooff
//         arrays y [B F T][ldy], w [9][C] (tap-major), b [C]
//   op 2  bottleneck tail   hdr = B, F, T, d, ldy, yoff, ldres, roff, ldo, ooff        (K = 4 d)
//         arrays y1 [B F T][ldy], w2 [9][K], b2 [K], w3 [d][K], b3 [d], res [B F T][ldres]
//   op 3  downsample 3x3    hdr = B, Fi, Ti, cin, N, sf, st, lda, aoff, ldo, ooff
//         arrays a [B Fi Ti][lda], w [N][cin][9] (torch layout), bias [N]
//   op 4  1x1 conv + ReLU   hdr = M, cin, N, has_res, lda, aoff, ldo, ooff
//         arrays a [M][lda], w [N][cin], bias [N], (res [M][N])
// The slices read start at channel yoff / aoff / roff of a row, the slice written at channel ooff
// of a row of ldo; results out [(M + 8)][ldo], M = the output positions.  Guard rows and guard
// columns must come back untouched.
#include <vector>

#include "../wespeaker_hubert_amd/csrc/gemini.h"
#include "../wespeaker_hubert_amd/csrc/kernels.h"
#include "../wespeaker_hubert_amd/csrc/pack.h"
#include "op_runner.h"

using namespace wsp;

namespace {

constexpr int kX3Variant = 7;  // the family's tile family (make_gemini)

bool slice_ok(int off, int width, int ld) { return off >= 0 && width > 0 && off + width <= ld && ld <= 8192; }

void run_case(Case& in) {
  const uint32_t op = in.op;
  Pool& pool = in.pool;
  hipStream_t s = in.stream;
  float* d0 = nullptr;
  size_t n0 = 0;
  auto plane_ok = [](int B, int F, int T) { return B > 0 && F > 0 && T > 0 && (long long)B * F * T < (1 << 20); };
  if (op == 1) {
    const int* h = in.h;
    const int B = h[0], F = h[1], T = h[2], C = h[3], ldy = h[4], yoff = h[5], ldo = h[6], ooff = h[7];
    BAD(plane_ok(B, F, T) && C > 0 && C <= 4096, "shape out of range");
    BAD(slice_ok(yoff, C, ldy) && slice_ok(ooff, C, ldo), "bad slices");
    const long long M = (long long)B * F * T;
    const std::vector<float> y = in.f32(M * ldy, "y"), w = in.f32(9LL * C, "w"), b = in.f32(C, "b");
    n0 = (size_t)(M + 8) * ldo;
    d0 = pool.filled(n0);
    in.guarded([&] {
      const GeminiDwArgs p{pool.up(y) + yoff, ldy, B, F, T, C, pool.up(w), pool.up(b), d0 + ooff, ldo};
      launch_gemini_dw(p, s);
    });
  } else if (op == 2) {
    const int* h = in.h;
    const int B = h[0], F = h[1], T = h[2], d = h[3], ldy = h[4], yoff = h[5], ldres = h[6], roff = h[7], ldo = h[8],
              ooff = h[9];
    BAD(plane_ok(B, F, T) && d > 0 && d <= 1024, "shape out of range");
    const int K = 4 * d;
    BAD(slice_ok(yoff, K, ldy) && slice_ok(roff, d, ldres) && slice_ok(ooff, d, ldo), "bad slices");
    const long long M = (long long)B * F * T;
    const std::vector<float> y1 = in.f32(M * ldy, "y1"), w2 = in.f32(9LL * K, "w2"), b2 = in.f32(K, "b2"),
                             w3 = in.f32((long long)d * K, "w3"), b3 = in.f32(d, "b3"), res = in.f32(M * ldres, "res");
    n0 = (size_t)(M + 8) * ldo;
    d0 = pool.filled(n0);
    in.guarded([&] {
      const GeminiTailArgs p{pool.up(y1) + yoff, ldy,         B,           F,
                             T,                  d,           pool.up(w2), pool.up(b2),
                             pool.up(pack::frag16(w3.data(), d, K, K)),    pool.up(b3),
                             pool.up(res) + roff, ldres,      d0 + ooff,   ldo};
      launch_gemini_tail(p, s);
    });
  } else if (op == 3) {
    const int* h = in.h;
    const int B = h[0], Fi = h[1], Ti = h[2], cin = h[3], N = h[4], sf = h[5], st = h[6], lda = h[7], aoff = h[8],
              ldo = h[9], ooff = h[10];
    BAD(plane_ok(B, Fi, Ti) && cin > 0 && cin <= 1024 && N > 0 && N <= 1024 && sf >= 1 && sf <= 4 && st >= 1 && st <= 4,
        "shape out of range");
    BAD(slice_ok(aoff, cin, lda) && slice_ok(ooff, N, ldo), "bad slices");
    const long long rows = (long long)B * Fi * Ti;
    const int Fo = (Fi - 1) / sf + 1, To = (Ti - 1) / st + 1, M = B * Fo * To;
    const std::vector<float> a = in.f32(rows * lda, "a"), w = in.f32((long long)N * cin * 9, "w"), bias = in.f32(N, "bias");
    n0 = (size_t)(M + 8) * ldo;
    d0 = pool.filled(n0);
    in.guarded([&] {
      const int K = 9 * cin;
      const std::vector<float> wk = pack::conv_kmajor(w, N, cin, 9, K);
      const GeminiDownArgs p{pool.up(a) + aoff, lda, B, Fi, Ti, cin, sf, st, pool.up(pack::frag16(wk.data(), N, K, K)),
                             pool.up(bias),     N,   d0 + ooff, ldo};
      launch_gemini_down(p, s);
    });
  } else if (op == 4) {
    const int* h = in.h;
    const int M = h[0], cin = h[1], N = h[2], has_res = h[3], lda = h[4], aoff = h[5], ldo = h[6], ooff = h[7];
    BAD(M > 0 && M < (1 << 20) && cin > 0 && cin <= 4096 && N > 0 && N <= 4096, "shape out of range");
    BAD(slice_ok(aoff, cin, lda) && slice_ok(ooff, N, ldo), "bad slices");
    const std::vector<float> a = in.f32((long long)M * lda, "a"), w = in.f32((long long)N * cin, "w"), bias = in.f32(N, "bias");
    std::vector<float> res;
    if (has_res) res = in.f32((long long)M * N, "res");
    n0 = (size_t)(M + 8) * ldo;
    d0 = pool.filled(n0);
    in.guarded([&] {
      // as Gemini::forward fills it (Impl::one_operand / fill): one dense segment, one "utterance" of M rows
      const int Kp = (cin + 63) / 64 * 64;
      std::vector<uint16_t> whi, wlo;
      pack::split(pack::conv_kmajor(w, N, cin, 1, Kp), whi, wlo);
      ConvGemmArgs g{};
      const float* da = pool.up(a) + aoff;
      g.a[0] = g.a[1] = g.a[2] = da;
      g.lda[0] = g.lda[1] = g.lda[2] = lda;
      g.cseg[1] = g.cseg[2] = g.cseg[3] = cin;
      g.cin = cin, g.taps = 1, g.dil = 1, g.pad = 0;
      g.M = M, g.T = M, g.N = N, g.K = cin, g.Kp = Kp;
      g.bias = pool.up(bias);
      g.out = d0 + ooff, g.ldo = ldo, g.act = kActRelu;
      if (has_res) g.res = pool.up(res), g.ldres = N, g.role = 2;
      launch_conv_gemm_x3(g, pool.up(whi), pool.up(wlo), kX3Variant, s);
    });
  } else {
    BAD(false, "unknown operator");
  }
  in.result(d0, n0);
}

}  // namespace

int main(int argc, char** argv) { return op_runner_main(argc, argv, "gemini_run", 0x47505357u, Layout{16, 0, 1}, run_case); }
