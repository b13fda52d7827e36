// Host-side weight packing arithmetic: plain C++ over std::vector, no HIP, so it builds
// and runs on its own (tools/pack_check.cpp).  Model::Impl packs with these, then uploads.
#pragma once

#include <cstdint>
#include <cstring>
#include <vector>

namespace wsp {
namespace pack {

// fp32 -> bf16, round to nearest even (matches v_cvt_pk_bf16_f32 on finite values)
inline uint16_t f2bf(float f) {
  uint32_t u;
  std::memcpy(&u, &f, 4);
  u += 0x7FFFu + ((u >> 16) & 1u);
  return (uint16_t)(u >> 16);
}
inline float bf2f(uint16_t b) {
  const uint32_t u = (uint32_t)b << 16;
  float f;
  std::memcpy(&f, &u, 4);
  return f;
}

// bf16x3 operand planes: hi = bf16(v), lo = bf16(v - hi)
void split(const std::vector<float>& v, std::vector<uint16_t>& hi, std::vector<uint16_t>& lo);

// Conv weight [N][cin][taps] -> [N][Kp] with k = tap * cin + c, zero tail (Kp >= cin * taps)
std::vector<float> conv_kmajor(const std::vector<float>& w, int N, int cin, int taps, int Kp);

// Linear weight [N][K] (row stride ldk) -> k-major [K][N]
std::vector<float> transpose(const float* w, int N, int K, int ldk);

// Weight [N][K] -> bf16 hi / lo in MFMA B-fragment order
// [K/16 k-steps][2 planes][N/32 column tiles][64 lanes][8].  Lane l, element e of k-step ks holds
// W[n = 32 j + (l & 31)][k], with k in one of two orders:
//   kPlain  k = 16 ks + 8 (l >> 5) + e: the B operand of a 32x32x16 MFMA
//   kAcc    k = 16 ks + (e & 3) + 8 (e >> 2) + 4 (l >> 5): the order in which a transposed 32x32
//           accumulator tile holds its 32 rows (register r = (r & 3) + 8 (r >> 2) + 4 (l >> 5)), so
//           such accumulators feed this weight's MFMAs as the A operand without a shuffle
//           (bottleneck_tail).  kacc >= 0: only the k-steps below kacc in that order, the rest
//           plain (the in-tail shortcut's x fragments, BottleneckTailArgs::xsc)
enum FragOrder { kPlain, kAcc };
std::vector<uint16_t> frag(const std::vector<float>& w, int N, int K, FragOrder order = kPlain, int kacc = -1);

// Weight [N][K] (row stride ldw) -> bf16 hi / lo operand fragments of 16x16x32 MFMAs, rows padded
// with zeros to Np = round_up(N, 16) and k to Kp = round_up(K, 32):
// [Kp/32 k-steps][2 planes][Np/16 tiles][64 lanes][8].  Lane l, element e of k-step ks and tile j
// holds W[16 j + (l & 15)][k], k = 32 ks + 8 (l >> 4) + e or, acc_order,
// k = 32 ks + 16 (e >> 2) + 4 (l >> 4) + (e & 3): the order in which two stacked 16x16 accumulator
// tiles (register r = row 4 (l >> 4) + r) hold their 32 rows, so such accumulators are the other
// operand of this weight's MFMAs without a shuffle (eres2net.hip, the AFF's second product)
std::vector<uint16_t> frag16(const float* w, int N, int K, int ldw, bool acc_order = false);

// Res2Net chain (res2_chain.hip): 7 conv weights W_i [w][w][3] -> [7] plain fragment images of
// [w][3w] with k = tap * w + c
std::vector<uint16_t> frag_res2(const std::vector<float>* const W[7], int w);

}  // namespace pack
}  // namespace wsp
