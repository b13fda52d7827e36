// HuBERT / WavLM self-attention with K / V staged once per key block in LDS (attn.hip).
#pragma once

#include "common.h"

namespace wsp {

// WavLM relative-position bias: the bucket of d = key - query is constant for |d| >= 778
// (bucket 159 / 319 of 160 + 160), so one table over d in [-778, 778] with the index clamped
// is exact.  Per head kAttnRelStride floats (1557 used, index d + 778).
constexpr int kAttnRelMax = 778;
constexpr int kAttnRelN = 2 * kAttnRelMax + 1;
constexpr int kAttnRelStride = 1560;

// Gated relative-position bias (WavLM): score(i, j) += gate[row i][head] * table[head][j - i].
struct AttnBias {
  const float* table = nullptr;  // device [H][kAttnRelStride]
  const float* gate = nullptr;   // device [rows][H] (launch_attn_gate)
};

// softmax(Q K^T / sqrt(dh) (+ bias)) V per (utterance, head); qkv [rows][ldq] = [q | k | v]
// (H*dh each), out [rows][ldo]; seg (device [B+1] row offsets) for ragged batches (bias
// positions are utterance-local).
// pipe = 1: the persistent pipelined kernel (default), 0: one block per (utterance, head).
// bias = nullptr runs the plain (HuBERT) instantiations.
void launch_attn(const float* qkv, int ldq, float* out, int ldo, int B, int T, int H, int dh, hipStream_t s,
                 const int* seg = nullptr, int pipe = 1, const AttnBias* bias = nullptr);

// WavLM gate per (row, head) from the layer input x [rows][ldx] (head h = columns 64 h .. 64 h + 63):
//   ga = sigmoid(x_h . wa + ba), gb = sigmoid(x_h . wb + bb), gate = ga * (gb * grep_a[h] - 1) + 2
// w (device) = [wa (64) | wb (64) | ba | bb | grep_a (H)]: grep_linear's rows 0..3 / 4..7 summed.
void launch_attn_gate(const float* x, int ldx, int rows, int H, const float* w, float* gate, hipStream_t s);

}  // namespace wsp
