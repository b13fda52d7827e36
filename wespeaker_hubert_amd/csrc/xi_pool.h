// XI pooling (Gaussian posterior inference, pooling_layers.py class XI, stddev = False) and the
// row-offset tables of unpadded ("valid") 1-D convs over ragged batches — xi_pool.hip.
#pragma once

#include "common.h"

namespace wsp {

// phi[b][c] = (sum_t s_t^2 x_t + exp(lp_c) m_c) / (sum_t s_t^2 + exp(lp_c)),  s_t = softplus(z[b][t][c])
// (beta 1, threshold 20: z > 20 -> s = z): the reference's softmax over the T frames' log-precisions
// 2 log s_t plus one prior entry lp_c = prior_logprec[c], applied to [x_t ..., m_c = prior_mean[c]].
// z [rows][ldz] logits and x [rows][ldx] activations, channels-last; utterance b owns rows
// [seg[b], seg[b+1]) (device int32 [B+1]) or, seg null, rows b*T .. b*T + T-1.  out [B][ldo]; only
// columns [0, C) of out are written.  C, ldz, ldx, ldo multiples of 4, pointers 16-byte aligned.
// s_t in f32, the weights s_t^2, both sums and the quotient in f64: a nonzero s_t (>= 1.4e-45, the
// smallest f32) squares to >= 2e-90, far inside f64; below z of about -103 expf(z), and with it s_t,
// is exactly 0 and the frame drops out.  The result is finite for every finite logit because the
// prior's weight exp(lp) > 0 is always in the denominator.  An utterance's frames are summed in an
// order that depends on its own length alone (wave w of the block takes frames w, w + 4, ...; the
// four partials are added in wave order), so a row does not depend on the batch it is in.
struct XiPoolArgs {
  const float* z;
  int ldz;
  const float* x;
  int ldx;
  const float* prior_mean;     // [C]
  const float* prior_logprec;  // [C]
  int B, T, C;
  const int* seg;  // null = uniform T
  float* out;
  int ldo;
};
void launch_xi_pool(const XiPoolArgs& p, hipStream_t s);

// out[k][b] = off[b] - b * shrink[k] for b = 0 .. B, k < n <= 4 (device int32 [n][B + 1]): the rows
// utterance b owns after unpadded convs that shorten every utterance by shrink[k] frames in all.
void launch_valid_conv_offsets(const int* off, int B, const int* shrink, int n, int* out, hipStream_t s);

}  // namespace wsp
