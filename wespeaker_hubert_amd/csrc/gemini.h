// Gemini DF-ResNet kernels (gemini.hip): the depthwise 3x3 conv of the inverted bottleneck, the
// bottleneck's tail (depthwise 3x3 + ReLU folded into the B operand of the 1x1 projection, with
// residual and ReLU) and the 3x3 downsample conv with separate frequency / time strides
// (gemini_dfresnet.py:30-119).  NHWC fp32 activations [B][F][T][C]; the two MFMA kernels run
// bf16x3 products (f32 accumulation) of 16x16x32 MFMAs with the weights as the A operand, as
// eres2net.hip does, so a lane owns consecutive channels of one position.
//
// 3x3 neighbours are read straight from global memory; a tap outside the utterance's own (F, T)
// plane reads zero, never the neighbouring row, plane or utterance.
#pragma once

#include "common.h"

namespace wsp {

// out[p][c] = relu( b[c] + sum_{tap = 0..8} w[tap][c] y[p + tap][c] ),  c < C
// p = (b F + f) T + t; tap = 3 kf + kt reads (f + kf - 1, t + kt - 1).  The sum is a chain of f32
// fmaf over taps 0..8 in that order starting from 0, the bias is added last.  w = [9][C] (BN2
// folded in), b = [C].  C in {128, 256, 512, 1024}; ldy, ldo >= C, multiples of 4 floats; y / out
// point at the first channel read / written; out does not alias y.
struct GeminiDwArgs {
  const float* y;
  int ldy;
  int B, F, T, C;
  const float* w;
  const float* b;
  float* out;
  int ldo;
};
bool gemini_dw_supported(int C);
void launch_gemini_dw(const GeminiDwArgs& p, hipStream_t s);

// out[p][n] = relu( b3[n] + res[p][n] + sum_k W3[n][k] h[p][k] ),  n < d, k < K = 4 d
// with h exactly launch_gemini_dw's expression on (y1, w2, b2), evaluated on the fly while the
// product's fragments are formed (same taps, same order, same fmaf): both routes feed identical h
// values to the product.  The product, residual and ReLU are launch_eres_pw's, so the tail equals
// launch_gemini_dw followed by launch_eres_pw bit for bit, without the 4d-wide tensor's write and
// read.  w3 = pack::frag16(W3 [d][K]).
// d in {32, 64, 128, 256}; ldy >= K, ldres, ldo >= d, multiples of 4 floats; out aliases neither
// y1 nor res.
struct GeminiTailArgs {
  const float* y1;
  int ldy;
  int B, F, T, d;
  const float* w2;  // [9][K]
  const float* b2;  // [K]
  const void* w3;
  const float* b3;  // [d]
  const float* res;
  int ldres;
  float* out;
  int ldo;
};
bool gemini_tail_supported(int d);
void launch_gemini_tail(const GeminiTailArgs& p, hipStream_t s);

// out[m][n] = bias[n] + sum_{tap, c} a(m, tap, c) W[n][tap cin + c],  n < N   (no activation)
// m = (b Fo + fo) To + to, Fo = (Fi - 1) / sf + 1, To = (Ti - 1) / st + 1; tap = 3 kf + kt reads
// input position (fo sf + kf - 1, to st + kt - 1), zero outside the plane.
// (sf, st) in {(2, 1), (2, 2)}; (cin, N) in {(32, 32), (32, 64), (64, 128), (128, 256)};
// w = pack::frag16(W [N][9 cin]) with k = tap cin + c (pack::conv_kmajor), bias = [N] (the folded BN).
struct GeminiDownArgs {
  const float* a;
  int lda;
  int B, Fi, Ti, cin, sf, st;
  const void* w;
  const float* bias;
  int N;
  float* out;
  int ldo;
};
bool gemini_down_supported(int cin, int N);
void launch_gemini_down(const GeminiDownArgs& p, hipStream_t s);

}  // namespace wsp
