// Res2Net kernel (res2net.hip): the tail of a BasicBlockRes2Net (res2net.py:66-93, scale 2) in one
// launch, on the transposed bf16x3 MFMAs of eres2net.h (weights = A operand, positions = B columns).
//
//   s   = clamp(b1 + conv3x3(y[:, :w]), 0, 20)                  (BatchNorm folded; never leaves the registers)
//   out = clamp(b3 + W3 [s | y[:, w:]] + res, 0, 20)            (N output channels)
//
// y = [M][ldy] rows of the block's conv1 output (2w channels, NHWC over [B][F][T], M = B F T), zero
// padding at the plane edge, no read across utterances.  w1 = pack::frag16(W1 [w][9 w], k = tap w + c),
// b1 = [w]; w3 = pack::frag16(W3 [N][2 w], acc_order), b3 = [N]: the 3x3 accumulators are conv3's B
// operand as they stand.  res (null: none) = [M][ldres], out = [M][ldo]: only columns [0, N) of rows
// [0, M) are written.  N % 4 == 0, every stride a multiple of 4 floats, every pointer 16-byte aligned,
// every operand below 2 GiB.  w in {16, 32, 64, 128, 256}.
#pragma once

#include "common.h"

namespace wsp {

struct Res2TailArgs {
  const float* y;
  int ldy;
  int B, F, T, w;
  const void* w1;
  const float* b1;
  const void* w3;
  const float* b3;
  int N;
  const float* res;
  int ldres;
  float* out;
  int ldo;
};
bool res2_tail_supported(int w);  // 16, 32, 64, 128, 256
void launch_res2_tail(const Res2TailArgs& p, hipStream_t s);

}  // namespace wsp
