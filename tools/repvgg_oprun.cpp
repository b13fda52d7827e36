// Op-level runner for the RepVGG / RepSPK kernels (tests/test_gpu_repvgg_op.py).
// Launches launch_rsbb_conv and launch_repvgg_stem of libwsp_hip.so, with weights packed by the library's own
// pack::conv_kmajor / pack::split in the live-tap order of repvgg.h (kRsbbTaps).  Framing, case and result
// files: tools/op_runner.h.  Magic 'WSPV' (0x56505357).  Arrays are f32; one result array per case.
//
//   op 1  RepSPK block conv + bias + ReLU   hdr = B, Fi, Ti, cin, N, stride, ldx, ldo, ooff
//         arrays x [B Fi Ti][ldx], w [N][cin][5][5] (torch layout; the runner packs its 17 live taps), bias [N]
//         results out [(M + 8)][ldo],  M = B Fo To; the columns written start at channel ooff of a row
//   op 2  stem                              hdr = B, T, F, C0, Cpad, taps (9, 17, 25), ldo, ooff
//         arrays feats [B][T][F], w [C0][k][k] (k = 3 for 9 taps, else 5; 17: the runner takes the live taps),
//         bias [C0];  results out [(M + 8)][ldo],  M = B F T
// Guard rows and guard columns must come back untouched.
#include <vector>

#include "../wespeaker_hubert_amd/csrc/pack.h"
#include "../wespeaker_hubert_amd/csrc/repvgg.h"
#include "op_runner.h"

using namespace wsp;

namespace {

// [n][5][5] per (n, c) pair -> [n][17] in live-tap order
std::vector<float> live_taps(const std::vector<float>& w5, size_t pairs) {
  std::vector<float> out(pairs * kRsbbLiveTaps);
  for (size_t i = 0; i < pairs; ++i)
    for (int j = 0; j < kRsbbLiveTaps; ++j) out[i * kRsbbLiveTaps + j] = w5[i * 25 + kRsbbTaps[j][0] * 5 + kRsbbTaps[j][1]];
  return out;
}

void run_case(Case& in) {
  const uint32_t op = in.op;
  Pool& pool = in.pool;
  hipStream_t s = in.stream;
  const int* h = in.h;
  float* d0 = nullptr;
  size_t n0 = 0;
  if (op == 1) {
    const int B = h[0], Fi = h[1], Ti = h[2], cin = h[3], N = h[4], stride = h[5], ldx = h[6], ldo = h[7], ooff = h[8];
    BAD(B > 0 && Fi > 0 && Ti > 0 && (long long)B * Fi * Ti < (1 << 20), "shape out of range");
    BAD(cin > 0 && cin <= 4096 && N > 0 && N <= 4096 && stride >= 1 && stride <= 4, "cin / N / stride out of range");
    // what the kernel may read or write if the launch is not refused stays inside the arrays
    BAD(ldx >= cin && ldx <= 8192 && ooff >= 0 && ooff + N <= ldo && ldo <= 8192, "bad slices");
    const int Fo = (Fi - 1) / stride + 1, To = (Ti - 1) / stride + 1, M = B * Fo * To;
    const std::vector<float> x = in.f32((long long)B * Fi * Ti * ldx, "x"), w = in.f32((long long)N * cin * 25, "w"),
                             bias = in.f32(N, "bias");
    n0 = (size_t)(M + 8) * ldo;
    d0 = pool.filled(n0);
    in.guarded([&] {
      const int K = kRsbbLiveTaps * cin, Kp = (K + 63) / 64 * 64;
      std::vector<uint16_t> hi, lo;
      pack::split(pack::conv_kmajor(live_taps(w, (size_t)N * cin), N, cin, kRsbbLiveTaps, Kp), hi, lo);
      const RsbbConvArgs p{pool.up(x), ldx, B, Fi, Ti, cin, stride, pool.up(hi), pool.up(lo), pool.up(bias), N, d0 + ooff, ldo};
      launch_rsbb_conv(p, s);
    });
  } else if (op == 2) {
    const int B = h[0], T = h[1], F = h[2], C0 = h[3], Cpad = h[4], taps = h[5], ldo = h[6], ooff = h[7];
    BAD(B > 0 && T > 0 && F > 0 && (long long)B * T * F < (1 << 20), "shape out of range");
    BAD(C0 > 0 && C0 <= 256 && taps > 0 && taps <= 25, "C0 / taps out of range");
    BAD(Cpad >= C0 && ooff >= 0 && ooff + Cpad <= ldo && ldo <= 8192, "bad slices");
    const int kk = taps == 9 ? 9 : 25, M = B * F * T;
    const std::vector<float> feats = in.f32((long long)M, "feats"), w = in.f32((long long)C0 * kk, "w"),
                             bias = in.f32(C0, "bias");
    n0 = (size_t)(M + 8) * ldo;
    d0 = pool.filled(n0);
    in.guarded([&] {
      const RepvggStemArgs p{pool.up(feats), B, T, F, C0, Cpad, taps, pool.up(taps == kRsbbLiveTaps ? live_taps(w, C0) : w),
                             pool.up(bias), d0 + ooff, ldo};
      launch_repvgg_stem(p, s);
    });
  } else {
    BAD(false, "unknown operator");
  }
  in.result(d0, n0);
}

}  // namespace

int main(int argc, char** argv) { return op_runner_main(argc, argv, "repvgg_oprun", 0x56505357u, Layout{12, 0, 1}, run_case); }
