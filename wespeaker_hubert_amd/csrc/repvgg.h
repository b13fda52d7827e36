// RepVGG / RepSPK kernels (repvgg.hip).
//
// launch_rsbb_conv: the folded RepSPK block (repvgg.py:289-453 after switch_to_deploy) as one conv +
// bias + ReLU over the 17 live taps of its 5x5 kernel,
//
//   out[b][fo][to][n] = relu(bias[n] + sum over the live taps (kf, kt), sum_c
//                            x[b][fo*s + kf - 2][to*s + kt - 2][c] * W[n][c][kf][kt])
//
// s = 1 or 2, zero padding 2, no read across utterances.  The 3x3 branch reaches the taps 1 <= kf, kt <= 3
// and the dilation-2 3x3 branch the taps with kf and kt both even; they share the centre, so 17 of the 25
// taps are live and the other eight are zero in every folded kernel.  They are neither loaded nor
// multiplied: the contraction is K = 17 cin.
//
// LIVE-TAP ORDER (kRsbbTaps): row-major over the 5x5 with the dead taps left out,
//   j :  0     1     2     3     4     5     6     7     8     9     10    11    12    13    14    15    16
//   kf:  0     0     0     1     1     1     2     2     2     2     2     3     3     3     4     4     4
//   kt:  0     2     4     1     2     3     0     1     2     3     4     1     2     3     0     2     4
// and the k order of the packed weight is (tap in live-tap order, c): whi / wlo = the bf16 hi / lo images
// of W as [N][Kp] with k = j * cin + c, Kp = round_up(17 cin, 64), zero tail (pack::conv_kmajor over
// [N][cin][17], then pack::split).  bf16x3 products with f32 accumulation in the conv-GEMM family's order
// (bf16x3.h mma3: lo*hi, hi*lo, hi*hi) and its epilogue (gemm_common.h).
//
// x = [B][Fi][Ti][ldx] (cin channels read), out = [M][ldo] with M = B Fo To, Fo = (Fi - 1) / s + 1, To
// alike; only columns [0, N) of rows [0, M) are written.  cin % 32 == 0, N % 32 == 0, ldx % 4 == 0,
// ldo % 4 == 0, x and out 16-byte aligned (the next layer reads the rows it writes with 16-byte loads),
// every operand below 2 GiB.  Block tile 128 rows x 128 / 64 / 32 columns (the widest that divides N).
//
// launch_repvgg_stem: stage0, the 1 -> C0 block of either kind with 9 (3x3, pad 1), 17 (live taps of the
// 5x5, pad 2) or 25 (the whole 5x5: a checkpoint whose dead taps are not zero) taps, + bias + ReLU in f32 FMAs.  Reads the (B, T, F) features as the (B, 1, F, T) image and
// writes NHWC [B][F][T][ldo]: channels [0, C0) the conv, channels [C0, Cpad) zeros (the channel padding of
// the widths the GEMMs do not take), nothing beyond.  w = [C0][taps] (3x3 / 5x5 row-major, or live-tap order),
// C0 in {32, 48, 64}, C0 <= Cpad <= ldo, Cpad % 4 == 0, ldo % 4 == 0, out 16-byte aligned.
#pragma once

#include "common.h"

namespace wsp {

constexpr int kRsbbLiveTaps = 17;
constexpr int kRsbbTaps[kRsbbLiveTaps][2] = {{0, 0}, {0, 2}, {0, 4}, {1, 1}, {1, 2}, {1, 3}, {2, 0}, {2, 1}, {2, 2},
                                             {2, 3}, {2, 4}, {3, 1}, {3, 2}, {3, 3}, {4, 0}, {4, 2}, {4, 4}};

struct RsbbConvArgs {
  const float* x;
  int ldx;
  int B, Fi, Ti, cin, stride;
  const void* whi;
  const void* wlo;
  const float* bias;
  int N;
  float* out;
  int ldo;
};
void launch_rsbb_conv(const RsbbConvArgs& p, hipStream_t s);

struct RepvggStemArgs {
  const float* feats;
  int B, T, F;
  int C0, Cpad, taps;
  const float* w;
  const float* bias;
  float* out;
  int ldo;
};
void launch_repvgg_stem(const RepvggStemArgs& p, hipStream_t s);

}  // namespace wsp
