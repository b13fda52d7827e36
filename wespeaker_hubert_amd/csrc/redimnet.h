// ReDimNet kernels (redimnet.hip; redimnet.py:47-619).  The activation is frame rows [B * T][1152]
// with column f * c + ch — the reference's 1-D view (to1d) and, read as [B][T][F][c], every stage's
// 2-D view, so neither reshape moves data.  All of them are f32 fmaf chains on f32 storage; row
// strides (ld*) are in floats and multiples of 4, base pointers 16-byte aligned.  No kernel may run
// in place: a block reads halo rows (or columns) that another block writes.
#pragma once

#include <hip/hip_runtime.h>

namespace wsp {

constexpr int kRdWidth = 1152;  // C * F = 16 * 72
constexpr int kRdMaxIn = 7;     // the stem's output and the six stages'

// Stem: Conv2d(1, 16, 3, "same") over (F, T) of feats [B][T][72], then the channels-first LayerNorm
// over the 16 channels of each (f, t) (biased variance, eps): out[b*T + t][f*16 + ch].
// w = [9][16] tap-major, tap = kf * 3 + kt.
struct RdStemArgs {
  const float* feats;
  int B, T, F;
  const float *w, *bias, *gamma, *beta;
  float eps;
  float* out;
  int ldo;
};
void launch_rd_stem(const RdStemArgs& p, hipStream_t s);

// Stage entry: x[row][j] = sum_i sw[i][j] * in[i][row][j] over the n earlier 1-D outputs (sw = the
// softmax of inputs_weights over its inputs axis, taken on the host), then the (s, 1) / stride
// (s, 1) conv, which in this layout is a row-local product on groups of gw = s * c contiguous
// floats: out[row][g*gw + co] = bias[co] + sum_k wt[k][co] * x[row][g*gw + k], wt k-major with
// k = kf * c + ci.  gw = 0: the weighted sum alone (the backbone's output).
struct RdEntryArgs {
  const float* in[kRdMaxIn];
  int ld_in, n;
  const float* sw;  // [n][1152]
  int rows, gw;
  const float *wt, *bias;
  float* out;
  int ldo;
};
void launch_rd_entry(const RdEntryArgs& p, hipStream_t s);

// 2-D ConvNeXt block in one launch: grouped 3x3 "same" conv over (F, T) with 4 channels per group
// (+ bias, BatchNorm folded in), erf GELU, 1x1 conv c -> c (+ bias), + x.  x = [B*T][F*c].
// wd = [(kf*3 + kt)*4 + ci][c] (ci within the group of the output channel), wp = [c][c] k-major.
struct RdBlock2dArgs {
  const float* x;
  int ldx, B, T, F, c;
  const float *wd, *bd, *wp, *bp;
  float* out;
  int ldo;
};
bool rd_block2d_supported(int F, int c);
void launch_rd_block2d(const RdBlock2dArgs& p, hipStream_t s);

// 1-D ConvNeXt block in one launch: depthwise conv over frames (k odd, <= 59, zero "same" padding,
// BatchNorm folded in), erf GELU, 1x1 conv C -> C, + x.  x = [B*T][C] (C <= 320, C % 4 == 0).
// wd = [k][C] tap-major, wp = [C][C] k-major.
struct RdBlock1dArgs {
  const float* x;
  int ldx, B, T, C, k;
  const float *wd, *bd, *wp, *bp;
  float* out;
  int ldo;
};
void launch_rd_block1d(const RdBlock1dArgs& p, hipStream_t s);

// out[m] = LayerNorm_D(x[m] (+ add[m])) * gamma + beta (biased variance), D <= 512.
struct RdLnArgs {
  const float* x;
  int ldx;
  const float* add;  // or null
  int ldadd;
  const float *gamma, *beta;
  float eps;
  float* out;
  int ldo, M, D;
};
void launch_rd_layernorm(const RdLnArgs& p, hipStream_t s);

// Multi-head self-attention over each utterance's T frames, no mask: qkv = [B*T][>= 3*H*dh] with q
// at column h*dh, k at H*dh + h*dh, v at 2*H*dh + h*dh; q is multiplied by `scale` here (after its
// bias, as the reference).  Keys stream in chunks of 32 with a running maximum: no [T][T] buffer.
// dh in {24, 36, 72}.
struct RdAttnArgs {
  const float* qkv;
  int ld, B, T, H, dh;
  float scale;
  float* out;
  int ldo;
};
bool rd_attn_supported(int dh);
void launch_rd_attn(const RdAttnArgs& p, hipStream_t s);

// x[m][0..D) = 0.5 x (1 + tanh(sqrt(2/pi) (x + 0.044715 x^3))) in place (the "NewGELU")
void launch_rd_gelu_tanh(float* x, int ldx, int M, int D, hipStream_t s);

}  // namespace wsp
