// Op-level runner for the Res2Net kernels (tests/test_gpu_res2net_op.py).
// Launches launch_res2_tail and launch_eres_pw / launch_eres_conv3x3 (with EresConvArgs::ksplit) of
// libwsp_hip.so, with weights packed by the library's own pack::frag16 / pack::conv_kmajor.  Framing,
// case and result files: tools/op_runner.h.  Magic 'WSP2' (0x32505357).  Arrays are f32; one result
// array per case.
//
//   op 1  fused block tail            hdr = B, F, T, w, N, ldy, ldo, ooff, has_res, ldres
//         arrays y [B F T][ldy], w1 [w][w][9] (torch layout), b1 [w], w3 [N][2w], b3 [N], (res [M][ldres])
//         results out [(M + 8)][ldo],  M = B F T; the columns written start at channel ooff of a row
//   op 2  conv with a concatenated operand   hdr = taps (1; 9 only to be refused), B, Fi, Ti, cin, N,
//         stride, ksplit, lda, lda2, ldo, ooff, act, has_res, null_a2
//         arrays a [B Fi Ti][lda], a2 [B Fi Ti][lda2], w [N][cin][taps], bias [N], (res [M][N])
//         results out [(M + 8)][ldo],  M = B Fo To
// Guard rows and guard columns must come back untouched.
#include <vector>

#include "../wespeaker_hubert_amd/csrc/eres2net.h"
#include "../wespeaker_hubert_amd/csrc/pack.h"
#include "../wespeaker_hubert_amd/csrc/res2net.h"
#include "op_runner.h"

using namespace wsp;

namespace {

void run_case(Case& in) {
  const uint32_t op = in.op;
  Pool& pool = in.pool;
  hipStream_t s = in.stream;
  const int* h = in.h;
  float* d0 = nullptr;
  size_t n0 = 0;
  if (op == 1) {
    const int B = h[0], F = h[1], T = h[2], w = h[3], N = h[4], ldy = h[5], ldo = h[6], ooff = h[7], has_res = h[8],
              ldres = h[9];
    BAD(B > 0 && F > 0 && T > 0 && (long long)B * F * T < (1 << 20), "shape out of range");
    BAD(w > 0 && w <= 1024 && N > 0 && N <= 4096, "w / N out of range");
    BAD(ldy >= 2 * w && ldy <= 8192 && ooff >= 0 && ooff + N <= ldo && ldo <= 8192, "bad slices");
    BAD(!has_res || (ldres >= N && ldres <= 8192), "bad residual stride");
    const int M = B * F * T;
    const std::vector<float> y = in.f32((long long)M * ldy, "y"), w1 = in.f32((long long)w * w * 9, "w1"),
                             b1 = in.f32(w, "b1"), w3 = in.f32((long long)N * 2 * w, "w3"), b3 = in.f32(N, "b3");
    std::vector<float> res;
    if (has_res) res = in.f32((long long)M * ldres, "res");
    n0 = (size_t)(M + 8) * ldo;
    d0 = pool.filled(n0);
    in.guarded([&] {
      const std::vector<float> wk = pack::conv_kmajor(w1, w, w, 9, 9 * w);
      Res2TailArgs p{pool.up(y), ldy, B, F, T, w, pool.up(pack::frag16(wk.data(), w, 9 * w, 9 * w)), pool.up(b1),
                     pool.up(pack::frag16(w3.data(), N, 2 * w, 2 * w, true)), pool.up(b3), N, nullptr, 0, d0 + ooff, ldo};
      if (has_res) p.res = pool.up(res), p.ldres = ldres;
      launch_res2_tail(p, s);
    });
  } else if (op == 2) {
    const int taps = h[0], B = h[1], Fi = h[2], Ti = h[3], cin = h[4], N = h[5], stride = h[6], ksplit = h[7], lda = h[8],
              lda2 = h[9], ldo = h[10], ooff = h[11], act = h[12], has_res = h[13], null_a2 = h[14];
    BAD((taps == 1 || taps == 9) && B > 0 && Fi > 0 && Ti > 0 && (long long)B * Fi * Ti < (1 << 20), "shape out of range");
    BAD(cin > 0 && cin <= 4096 && N > 0 && N <= 4096 && (stride == 1 || stride == 2), "cin / N / stride out of range");
    BAD(lda > 0 && lda <= 8192 && lda2 > 0 && lda2 <= 8192 && ksplit >= -64 && ksplit <= 8192, "bad input strides");
    // what the kernel may read if the launch is not refused stays inside the arrays
    BAD(lda >= cin && lda2 >= cin, "input rows shorter than cin");
    BAD(ooff >= 0 && ooff + N <= ldo && ldo <= 8192, "bad output slice");
    const long long rows = (long long)B * Fi * Ti;
    const int Fo = (Fi - 1) / stride + 1, To = (Ti - 1) / stride + 1, M = B * Fo * To;
    const std::vector<float> a = in.f32(rows * lda, "a"), a2 = in.f32(rows * lda2, "a2"),
                             w = in.f32((long long)N * cin * taps, "w"), bias = in.f32(N, "bias");
    std::vector<float> res;
    if (has_res) res = in.f32((long long)M * N, "res");
    n0 = (size_t)(M + 8) * ldo;
    d0 = pool.filled(n0);
    in.guarded([&] {
      const int K = cin * taps;
      const std::vector<float> wk = pack::conv_kmajor(w, N, cin, taps, K);
      EresConvArgs p{pool.up(a), lda, null_a2 ? nullptr : pool.up(a2), lda2, B, Fi, Ti, cin, stride,
                     pool.up(pack::frag16(wk.data(), N, K, K)), pool.up(bias), N, nullptr, 0, d0 + ooff, ldo, act, ksplit};
      if (has_res) p.res = pool.up(res), p.ldres = N;
      if (taps == 9)
        launch_eres_conv3x3(p, s);
      else
        launch_eres_pw(p, s);
    });
  } else {
    BAD(false, "unknown operator");
  }
  in.result(d0, n0);
}

}  // namespace

int main(int argc, char** argv) { return op_runner_main(argc, argv, "res2net_oprun", 0x32505357u, Layout{16, 0, 1}, run_case); }
