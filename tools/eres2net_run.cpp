// Op-level runner for the ERes2Net kernels (tests/test_gpu_eres2net_op.py).
// Launches launch_eres_conv3x3, launch_eres_pw and launch_eres_aff of libwsp_hip.so, with weights
// packed by the library's own pack::frag16 / pack::conv_kmajor.  Framing, case and result files:
// tools/op_runner.h.  Magic 'WSPE' (0x45505357).  Arrays are f32; one result array per case.
//
//   op 1  conv (3x3 Res2 step / 1x1)   hdr = taps (9 or 1), B, Fi, Ti, cin, N, stride, lda, aoff,
//         a2off (-1: no added slice), ldo, ooff, act, has_res
//         arrays a [B Fi Ti][lda], (a2 [B Fi Ti][lda]), w [N][cin][taps] (torch layout), bias [N],
//         (res [M][N]);  the slices read start at channel aoff / a2off of a row, the slice written at
//         channel ooff of a row of ldo;  results out [(M + 8)][ldo],  M = B Fo To
//   op 2  AFF                          hdr = M, C, ldx, xoff, ldy, yoff, ldo, ooff
//         arrays x [M][ldx], y [M][ldy], wa [C/4][2C], ba [C/4], wb [C][C/4], bb [C]
//         results out [(M + 8)][ldo]
// Guard rows and guard columns must come back untouched.
#include <algorithm>
#include <vector>

#include "../wespeaker_hubert_amd/csrc/eres2net.h"
#include "../wespeaker_hubert_amd/csrc/pack.h"
#include "op_runner.h"

using namespace wsp;

namespace {

void run_case(Case& in) {
  const uint32_t op = in.op;
  Pool& pool = in.pool;
  hipStream_t s = in.stream;
  float* d0 = nullptr;
  size_t n0 = 0;
  if (op == 1) {
    const int* h = in.h;
    const int taps = h[0], B = h[1], Fi = h[2], Ti = h[3], cin = h[4], N = h[5], stride = h[6], lda = h[7], aoff = h[8],
              a2off = h[9], ldo = h[10], ooff = h[11], act = h[12], has_res = h[13];
    BAD((taps == 1 || taps == 9) && B > 0 && Fi > 0 && Ti > 0 && (long long)B * Fi * Ti < (1 << 20), "shape out of range");
    BAD(cin > 0 && cin <= 4096 && N > 0 && N <= 4096 && (stride == 1 || stride == 2), "cin / N / stride out of range");
    BAD(aoff >= 0 && aoff + cin <= lda && lda <= 8192 && a2off >= -1 && a2off + cin <= lda, "bad input slice");
    BAD(ooff >= 0 && ooff + N <= ldo && ldo <= 8192, "bad output slice");
    const long long rows = (long long)B * Fi * Ti;
    const int Fo = (Fi - 1) / stride + 1, To = (Ti - 1) / stride + 1, M = B * Fo * To;
    const std::vector<float> a = in.f32(rows * lda, "a");
    std::vector<float> a2, res;
    if (a2off >= 0) a2 = in.f32(rows * lda, "a2");
    const std::vector<float> w = in.f32((long long)N * cin * taps, "w"), bias = in.f32(N, "bias");
    if (has_res) res = in.f32((long long)M * N, "res");
    n0 = (size_t)(M + 8) * ldo;
    d0 = pool.filled(n0);
    in.guarded([&] {
      const int K = cin * taps;
      const std::vector<float> wk = pack::conv_kmajor(w, N, cin, taps, K);
      EresConvArgs p{pool.up(a) + aoff, lda, nullptr, 0,   B,   Fi,   Ti, cin, stride, pool.up(pack::frag16(wk.data(), N, K, K)),
                     pool.up(bias),     N,   nullptr, 0,   d0 + ooff, ldo, act};
      if (a2off >= 0) p.a2 = pool.up(a2) + a2off, p.lda2 = lda;
      if (has_res) p.res = pool.up(res), p.ldres = N;
      if (taps == 9)
        launch_eres_conv3x3(p, s);
      else
        launch_eres_pw(p, s);
    });
  } else if (op == 2) {
    const int* h = in.h;
    const int M = h[0], C = h[1], ldx = h[2], xoff = h[3], ldy = h[4], yoff = h[5], ldo = h[6], ooff = h[7];
    BAD(M > 0 && M < (1 << 20) && C >= 4 && C <= 4096 && C % 4 == 0, "M / C out of range");
    BAD(xoff >= 0 && xoff + C <= ldx && ldx <= 8192 && yoff >= 0 && yoff + C <= ldy && ldy <= 8192, "bad input slices");
    BAD(ooff >= 0 && ooff + C <= ldo && ldo <= 8192, "bad output slice");
    const int H = C / 4, Hp = (H + 31) / 32 * 32;
    const std::vector<float> x = in.f32((long long)M * ldx, "x"), y = in.f32((long long)M * ldy, "y"),
                             wa = in.f32((long long)H * 2 * C, "wa"), ba = in.f32(H, "ba"),
                             wb = in.f32((long long)C * H, "wb"), bb = in.f32(C, "bb");
    n0 = (size_t)(M + 8) * ldo;
    d0 = pool.filled(n0);
    in.guarded([&] {
      // rows / columns [H, Hp) zero, as the model's fold_aff lays them out
      std::vector<float> wap((size_t)Hp * 2 * C, 0.f), bap(Hp, 0.f), wbp((size_t)C * Hp, 0.f);
      std::copy(wa.begin(), wa.end(), wap.begin());
      std::copy(ba.begin(), ba.end(), bap.begin());
      for (int n = 0; n < C; ++n) std::copy(wb.begin() + (size_t)n * H, wb.begin() + (size_t)(n + 1) * H, wbp.begin() + (size_t)n * Hp);
      const EresAffArgs p{pool.up(x) + xoff, ldx, pool.up(y) + yoff, ldy, M, C,
                          pool.up(pack::frag16(wap.data(), Hp, 2 * C, 2 * C)), pool.up(bap),
                          pool.up(pack::frag16(wbp.data(), C, Hp, Hp, true)), pool.up(bb), d0 + ooff, ldo};
      launch_eres_aff(p, s);
    });
  } else {
    BAD(false, "unknown operator");
  }
  in.result(d0, n0);
}

}  // namespace

int main(int argc, char** argv) { return op_runner_main(argc, argv, "eres2net_run", 0x45505357u, Layout{16, 0, 1}, run_case); }
