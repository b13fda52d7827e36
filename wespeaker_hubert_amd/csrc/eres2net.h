// ERes2Net kernels (eres2net.hip): the narrow 3x3 conv of the Res2 chain, the pointwise (1x1)
// conv with the clamp epilogue and the whole AFF gate in one launch (eres2net.py:75-240), all on
// bf16x3 products (hi*hi + hi*lo + lo*hi, f32 accumulation) of 16x16x32 MFMAs.
//
// The kernels run the MFMAs "transposed": the weights are the A operand (rows = output
// channels) and the activations the B operand (columns = positions), so a lane's four accumulator
// registers are four consecutive channels of one position: bias, residual and output move as
// 16-byte vectors, and an accumulator tile feeds the next product as its B operand without
// leaving the registers (the AFF's hidden row).
#pragma once

#include "common.h"

namespace wsp {

enum EresAct { kEresNone = 0, kEresRelu = 1, kEresClamp = 2 };  // clamp: min(max(y, 0), 20) (Hardtanh(0, 20))

// out[m][n] = act( bias[n] + res[m][n] + sum_{tap, c} A(m, tap, c) W[n][tap * cin + c] ), n < N
// Rows m = (b Fo + fo) To + to over NHWC tensors [B][Fi][Ti] of row stride lda (a, and a2 when
// non-null, point at the first channel of the slice read): A = a (+ a2) at input position
// (fo stride + kf - pad, to stride + kt - pad), zero outside the plane; tap = 3 kf + kt.
// taps = 9: pad 1 (launch_eres_conv3x3: stride 1, N == cin, the Res2 step); taps = 1: pad 0
// (launch_eres_pw: the 1x1 convs, stride 1 or 2).  cin % 8 == 0, N % 4 == 0; every stride and the
// channel offsets multiples of 4 floats.  w = pack::frag16(W [N][taps cin]), bias = [N].
// out / res point at the first channel written / read (row strides ldo / ldres): only columns
// [0, N) of rows [0, M) are written.
// launch_eres_pw with ksplit > 0 reads a concatenated operand instead of an added one: input channel
// k < ksplit is a[row][k], channel k >= ksplit is a2[row][k - ksplit] (row stride lda2); ksplit a
// multiple of 8 below cin, so a lane's eight consecutive k stay in one source (Res2Net's conv3 over
// [S | Y1[:, w:]]).  0 = off.
struct EresConvArgs {
  const float* a;
  int lda;
  const float* a2;
  int lda2;
  int B, Fi, Ti, cin, stride;
  const void* w;
  const float* bias;
  int N;
  const float* res;
  int ldres;
  float* out;
  int ldo;
  int act;
  int ksplit = 0;
};
bool eres_conv3x3_supported(int width);  // 16, 24, 32, 48, 64, 96, 128, 192, 256
void launch_eres_conv3x3(const EresConvArgs& p, hipStream_t s);
void launch_eres_pw(const EresConvArgs& p, hipStream_t s);

// AFF (eres2net.py:75-103) with both BatchNorms folded into the convs, one launch:
//   h = silu(Wa [x | y] + ba)   (H = C / 4 hidden channels, kept in registers)
//   g = 1 + tanh(Wb h + bb),  out = x g + y (2 - g)
// x, y, out = [M][ld] rows (slices or dense tensors), C channels each; out aliases neither input.
// With Hp = round_up(H, 32), rows / columns [H, Hp) zero: wa = pack::frag16(Wa [Hp][2C]),
// ba = [Hp], wb = pack::frag16(Wb [C][Hp], acc_order), bb = [C].
// C in {64, 96, 128, 192, 256, 512, 1024, 2048}.
struct EresAffArgs {
  const float* x;
  int ldx;
  const float* y;
  int ldy;
  int M, C;
  const void* wa;
  const float* ba;
  const void* wb;
  const float* bb;
  float* out;
  int ldo;
};
bool eres_aff_supported(int C);
void launch_eres_aff(const EresAffArgs& p, hipStream_t s);

}  // namespace wsp
