// CAM++ FCM head: the 3x3 convs strided in frequency only (fcm_conv.hip).
#pragma once

#include "common.h"

namespace wsp {

// out[b][fo][t][n] = act(bias[n] + sum_{kf, kt, c} x[b][2 fo + kf - 1][t + kt - 1][c] W[n][c][kf][kt])
// — Conv2d(32, 32, 3, stride (2, 1), padding 1) with its BatchNorm folded into W / bias, NHWC fp32,
// Fo = (Fi - 1) / 2 + 1, bf16x3 products.  w = cam_pack_b of [32][288] with k = (kf * 3 + kt) * 32 + c.
// tfc: the output is written as frame rows [B][T][Fo][32] (the TDNN's channels-last input).
// wsc non-null: also the block's projection shortcut, Conv2d(32, 32, 1, stride (2, 1)) + folded BN,
// from the centre tap's fragments: sc[b][fo][t][n] = bsc[n] + sum_c x[b][2 fo][t][c] Wsc[n][c]
// (no activation), wsc = cam_pack_b of [32][32].
struct FcmConvArgs {
  const float* x;
  float* out;
  int B, Fi, T;
  const void* w;
  const float* bias;
  int relu;
  int tfc;
  const void* wsc;
  const float* bsc;
  float* sc;
};
void launch_fcm_conv(const FcmConvArgs& p, hipStream_t s);

}  // namespace wsp
