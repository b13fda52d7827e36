#include "pack.h"

namespace wsp {
namespace pack {

void split(const std::vector<float>& v, std::vector<uint16_t>& hi, std::vector<uint16_t>& lo) {
  hi.resize(v.size());
  lo.resize(v.size());
  for (size_t i = 0; i < v.size(); ++i) {
    hi[i] = f2bf(v[i]);
    lo[i] = f2bf(v[i] - bf2f(hi[i]));
  }
}

std::vector<float> conv_kmajor(const std::vector<float>& w, int N, int cin, int taps, int Kp) {
  std::vector<float> packed((size_t)N * Kp, 0.f);
  for (int n = 0; n < N; ++n)
    for (int c = 0; c < cin; ++c)
      for (int j = 0; j < taps; ++j) packed[(size_t)n * Kp + j * cin + c] = w[((size_t)n * cin + c) * taps + j];
  return packed;
}

std::vector<float> transpose(const float* w, int N, int K, int ldk) {
  std::vector<float> t((size_t)K * N);
  for (int n = 0; n < N; ++n)
    for (int k = 0; k < K; ++k) t[(size_t)k * N + n] = w[(size_t)n * ldk + k];
  return t;
}

namespace {
// the one fragment loop: src(n, k) is the weight element, dst one [K/16][2][N/32][64][8] image
template <typename Src>
void frag_into(uint16_t* dst, int N, int K, FragOrder order, int kacc, Src src) {
  const int KS = K / 16, NT = N / 32;
  for (int ks = 0; ks < KS; ++ks)
    for (int jt = 0; jt < NT; ++jt)
      for (int l = 0; l < 64; ++l)
        for (int e = 0; e < 8; ++e) {
          const bool acc = order == kAcc && (kacc < 0 || ks * 16 < kacc);
          const int k = ks * 16 + (acc ? (e & 3) + 8 * (e >> 2) + 4 * (l >> 5) : 8 * (l >> 5) + e);
          const float v = src(jt * 32 + (l & 31), k);
          const uint16_t hi = f2bf(v);
          const size_t o = (((size_t)ks * 2 * NT + jt) * 64 + l) * 8 + e;
          dst[o] = hi;
          dst[o + (size_t)NT * 64 * 8] = f2bf(v - bf2f(hi));
        }
}
}  // namespace

std::vector<uint16_t> frag(const std::vector<float>& w, int N, int K, FragOrder order, int kacc) {
  std::vector<uint16_t> pk((size_t)(K / 16) * 2 * (N / 32) * 64 * 8);
  frag_into(pk.data(), N, K, order, kacc, [&](int n, int k) { return w[(size_t)n * K + k]; });
  return pk;
}

std::vector<uint16_t> frag16(const float* w, int N, int K, int ldw, bool acc_order) {
  const int NT = (N + 15) / 16, KS = (K + 31) / 32;
  std::vector<uint16_t> pk((size_t)KS * 2 * NT * 64 * 8, 0);
  for (int ks = 0; ks < KS; ++ks)
    for (int jt = 0; jt < NT; ++jt)
      for (int l = 0; l < 64; ++l)
        for (int e = 0; e < 8; ++e) {
          const int n = 16 * jt + (l & 15);
          const int k = 32 * ks + (acc_order ? 16 * (e >> 2) + 4 * (l >> 4) + (e & 3) : 8 * (l >> 4) + e);
          if (n >= N || k >= K) continue;
          const float v = w[(size_t)n * ldw + k];
          const uint16_t hi = f2bf(v);
          const size_t o = (((size_t)ks * 2 * NT + jt) * 64 + l) * 8 + e;
          pk[o] = hi;
          pk[o + (size_t)NT * 64 * 8] = f2bf(v - bf2f(hi));
        }
  return pk;
}

std::vector<uint16_t> frag_res2(const std::vector<float>* const W[7], int w) {
  const size_t per = (size_t)(3 * w / 16) * 2 * (w / 32) * 64 * 8;
  std::vector<uint16_t> pk(7 * per);
  for (int i = 0; i < 7; ++i)
    frag_into(pk.data() + i * per, w, 3 * w, kPlain, -1,
              [&](int n, int k) { return (*W[i])[((size_t)n * w + k % w) * 3 + k / w]; });
  return pk;
}

}  // namespace pack
}  // namespace wsp
