// Stand-alone check of the host weight packers (wespeaker_hubert_amd/csrc/pack.{h,cpp}): plain
// C++, no HIP, no GPU.  Every packer is compared with the inverse of its documented layout: for
// each weight element (n, k) the slot it must land in is computed here and both bf16 planes are
// compared, and every other slot must be untouched.  tests/test_pack_cpu.py builds this with
// -fsanitize=address,undefined and runs it.
//   c++ -std=c++17 -I wespeaker_hubert_amd/csrc tools/pack_check.cpp wespeaker_hubert_amd/csrc/pack.cpp
#include <cmath>
#include <cstdio>
#include <cstdlib>

#include "pack.h"

using namespace wsp::pack;

static int g_fail = 0;
#define CHECK(cond, ...)            \
  do {                              \
    if (!(cond)) {                  \
      if (++g_fail <= 20) {         \
        std::printf("FAIL %s:%d: ", __FILE__, __LINE__); \
        std::printf(__VA_ARGS__);   \
        std::printf("\n");          \
      }                             \
    }                               \
  } while (0)

static float from_bits(uint32_t u) {
  float f;
  std::memcpy(&f, &u, 4);
  return f;
}

// distinct values whose lo plane is non-zero and distinct too
static float value(size_t i) { return (i % 2 ? -1.f : 1.f) * (0.37f + 1.000123f * (float)(i % 9973) + 1e-4f * (float)(i % 7)); }

// k -> (lane half, element) within a 16-wide k-step
static void plain_slot(int r, int* half, int* e) {
  *half = r >> 3;
  *e = r & 7;
}
static void acc_slot(int r, int* half, int* e) {  // r = (e & 3) + 8 (e >> 2) + 4 half
  *half = (r >> 2) & 1;
  *e = (r & 3) + 4 * (r >> 3);
}

// One fragment image [K/16][2][N/32][64][8] against elem(n, k); acc_below: k-steps starting below
// it are in accumulator order.
template <typename Elem>
static void check_frag(const char* what, const uint16_t* pk, int N, int K, int acc_below, Elem elem) {
  const int NT = N / 32;
  const size_t total = (size_t)(K / 16) * 2 * NT * 64 * 8;
  std::vector<int> seen(total, 0);
  for (int n = 0; n < N; ++n)
    for (int k = 0; k < K; ++k) {
      const int ks = k / 16;
      int half, e;
      if (ks * 16 < acc_below) acc_slot(k % 16, &half, &e);
      else plain_slot(k % 16, &half, &e);
      const size_t hi_at = ((((size_t)ks * 2 + 0) * NT + n / 32) * 64 + (n % 32) + 32 * half) * 8 + e;
      const size_t lo_at = ((((size_t)ks * 2 + 1) * NT + n / 32) * 64 + (n % 32) + 32 * half) * 8 + e;
      const float v = elem(n, k);
      const uint16_t hi = f2bf(v), lo = f2bf(v - bf2f(hi));
      CHECK(pk[hi_at] == hi, "%s hi plane n=%d k=%d: %04x != %04x", what, n, k, pk[hi_at], hi);
      CHECK(pk[lo_at] == lo, "%s lo plane n=%d k=%d: %04x != %04x", what, n, k, pk[lo_at], lo);
      ++seen[hi_at];
      ++seen[lo_at];
    }
  for (size_t i = 0; i < total; ++i) CHECK(seen[i] == 1, "%s slot %zu is the target of %d elements", what, i, seen[i]);
}

static void test_frag(int N, int K, FragOrder order, int kacc) {
  std::vector<float> w((size_t)N * K);
  for (size_t i = 0; i < w.size(); ++i) w[i] = value(i);
  const std::vector<uint16_t> pk = frag(w, N, K, order, kacc);
  char what[64];
  std::snprintf(what, sizeof what, "frag %dx%d order %d kacc %d", N, K, (int)order, kacc);
  CHECK(pk.size() == (size_t)2 * N * K, "%s: %zu halves", what, pk.size());
  if (pk.size() != (size_t)2 * N * K) return;
  const int acc_below = order == kPlain ? 0 : kacc < 0 ? K : kacc;
  check_frag(what, pk.data(), N, K, acc_below, [&](int n, int k) { return w[(size_t)n * K + k]; });
}

// frag16 image [Kp/32][2][Np/16][64][8] of a [N][K] window (row stride ldw): every (n, k) in its
// slot, every padding slot zero
static void test_frag16(int N, int K, int ldw, bool acc) {
  std::vector<float> w((size_t)N * ldw);
  for (size_t i = 0; i < w.size(); ++i) w[i] = value(i);
  const std::vector<uint16_t> pk = frag16(w.data(), N, K, ldw, acc);
  const int NT = (N + 15) / 16, KS = (K + 31) / 32;
  const size_t total = (size_t)KS * 2 * NT * 64 * 8;
  char what[64];
  std::snprintf(what, sizeof what, "frag16 %dx%d ld %d acc %d", N, K, ldw, (int)acc);
  CHECK(pk.size() == total, "%s: %zu halves", what, pk.size());
  if (pk.size() != total) return;
  std::vector<int> seen(total, 0);
  for (int n = 0; n < N; ++n)
    for (int k = 0; k < K; ++k) {
      const int ks = k / 32, r = k % 32;
      // plain: r = 8 q + e; acc: r = 16 (e >> 2) + 4 q + (e & 3)
      const int q = acc ? (r >> 2) & 3 : r >> 3, e = acc ? 4 * (r >> 4) + (r & 3) : r & 7;
      const size_t hi_at = ((((size_t)ks * 2 + 0) * NT + n / 16) * 64 + (n % 16) + 16 * q) * 8 + e;
      const size_t lo_at = hi_at + (size_t)NT * 64 * 8;
      const float v = w[(size_t)n * ldw + k];
      const uint16_t hi = f2bf(v), lo = f2bf(v - bf2f(hi));
      CHECK(pk[hi_at] == hi, "%s hi plane n=%d k=%d: %04x != %04x", what, n, k, pk[hi_at], hi);
      CHECK(pk[lo_at] == lo, "%s lo plane n=%d k=%d: %04x != %04x", what, n, k, pk[lo_at], lo);
      ++seen[hi_at];
      ++seen[lo_at];
    }
  for (size_t i = 0; i < total; ++i) {
    CHECK(seen[i] <= 1, "%s slot %zu is the target of %d elements", what, i, seen[i]);
    if (!seen[i]) CHECK(pk[i] == 0, "%s padding slot %zu holds %04x", what, i, pk[i]);
  }
}

static void test_res2(int w) {
  std::vector<float> W[7];
  const std::vector<float>* Wp[7];
  for (int i = 0; i < 7; ++i) {
    W[i].resize((size_t)w * w * 3);
    for (size_t j = 0; j < W[i].size(); ++j) W[i][j] = value(j + 1000003u * i);
    Wp[i] = &W[i];
  }
  const std::vector<uint16_t> pk = frag_res2(Wp, w);
  const size_t per = (size_t)2 * w * 3 * w;
  CHECK(pk.size() == 7 * per, "res2 w=%d: %zu halves", w, pk.size());
  if (pk.size() != 7 * per) return;
  char what[32];
  for (int i = 0; i < 7; ++i) {
    std::snprintf(what, sizeof what, "res2 w=%d conv %d", w, i);
    // k = tap * w + c of W_i [n][c][tap]
    check_frag(what, pk.data() + i * per, w, 3 * w, 0, [&](int n, int k) { return W[i][((size_t)n * w + k % w) * 3 + k / w]; });
  }
}

static void test_conv_kmajor() {
  const int N = 3, cin = 5, taps = 3, Kp = 64;
  std::vector<float> w((size_t)N * cin * taps);
  for (size_t i = 0; i < w.size(); ++i) w[i] = value(i);
  const std::vector<float> p = conv_kmajor(w, N, cin, taps, Kp);
  CHECK(p.size() == (size_t)N * Kp, "conv_kmajor size %zu", p.size());
  if (p.size() != (size_t)N * Kp) return;
  for (int n = 0; n < N; ++n) {
    for (int c = 0; c < cin; ++c)
      for (int j = 0; j < taps; ++j)
        CHECK(p[(size_t)n * Kp + j * cin + c] == w[((size_t)n * cin + c) * taps + j], "conv_kmajor n=%d c=%d tap=%d", n, c, j);
    for (int k = cin * taps; k < Kp; ++k) CHECK(p[(size_t)n * Kp + k] == 0.f, "conv_kmajor tail n=%d k=%d", n, k);
  }
}

static void test_transpose() {
  const int N = 5, K = 7, ldk = 11;  // a [N][K] window of a wider row-major matrix
  std::vector<float> w((size_t)N * ldk);
  for (size_t i = 0; i < w.size(); ++i) w[i] = value(i);
  const std::vector<float> t = transpose(w.data(), N, K, ldk);
  CHECK(t.size() == (size_t)N * K, "transpose size %zu", t.size());
  if (t.size() != (size_t)N * K) return;
  for (int n = 0; n < N; ++n)
    for (int k = 0; k < K; ++k) CHECK(t[(size_t)k * N + n] == w[(size_t)n * ldk + k], "transpose n=%d k=%d", n, k);
}

static void test_bf16() {
  // {input bits, expected bf16}: round to nearest, ties to even
  const uint32_t cases[][2] = {
      {0x3F800000u, 0x3F80},  // 1.0 exactly
      {0x3F808000u, 0x3F80},  // tie, even below: down
      {0x3F818000u, 0x3F82},  // tie, odd below: up
      {0x3F808001u, 0x3F81},  // just above a tie: up
      {0x3F807FFFu, 0x3F80},  // just below a tie: down
      {0xBF808000u, 0xBF80},  // negative tie: to even, sign kept
      {0xBF818000u, 0xBF82},
      {0xBF808001u, 0xBF81},
      {0x3FFFFFFFu, 0x4000},  // mantissa carry into the exponent: 2.0
      {0xC07FC000u, 0xC080},  // negative carry: -4.0
      {0x00000000u, 0x0000},
      {0x80000000u, 0x8000},  // -0
  };
  for (const auto& c : cases) {
    const uint16_t got = f2bf(from_bits(c[0]));
    CHECK(got == c[1], "f2bf(%08x) = %04x, expected %04x", c[0], got, c[1]);
  }
  for (uint32_t b = 0; b < 0x10000u; b += 257) {  // bf16 -> f32 -> bf16 is the identity off NaN
    if ((b & 0x7F80u) == 0x7F80u) continue;
    CHECK(f2bf(bf2f((uint16_t)b)) == b, "bf16 round trip %04x", b);
  }
  std::vector<float> v(4096);
  for (size_t i = 0; i < v.size(); ++i) v[i] = value(i) * std::ldexp(1.f, (int)(i % 41) - 20);
  std::vector<uint16_t> hi, lo;
  split(v, hi, lo);
  CHECK(hi.size() == v.size() && lo.size() == v.size(), "split sizes");
  if (hi.size() != v.size() || lo.size() != v.size()) return;
  for (size_t i = 0; i < v.size(); ++i) {
    CHECK(hi[i] == f2bf(v[i]), "split hi %zu", i);
    const double err = std::fabs((double)v[i] - ((double)bf2f(hi[i]) + (double)bf2f(lo[i])));
    CHECK(err <= std::ldexp(std::fabs((double)v[i]), -16), "hi + lo of %g is off by %g", v[i], err);
  }
}

int main() {
  test_bf16();
  test_conv_kmajor();
  test_transpose();
  test_frag(32, 16, kPlain, -1);
  test_frag(64, 48, kPlain, -1);
  test_frag(128, 64, kAcc, -1);
  test_frag(128, 64, kAcc, 32);
  test_frag16(16, 144, 144, false);  // K padded to 160
  test_frag16(24, 216, 216, false);  // N padded to 32, K to 224
  test_frag16(72, 64, 80, false);    // a window of wider rows, N padded to 80
  test_frag16(64, 32, 32, true);
  test_frag16(96, 64, 70, true);
  test_res2(32);
  test_res2(64);
  if (g_fail) {
    std::printf("pack_check: %d failures\n", g_fail);
    return 1;
  }
  std::printf("pack_check: ok\n");
  return 0;
}
