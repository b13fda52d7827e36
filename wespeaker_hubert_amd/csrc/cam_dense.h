// CAM++ dense-TDNN kernels (cam_dense.hip): the BN-ReLU-prologue GEMM, the context mask and the
// masked local conv of a CAMDenseTDNNLayer (campplus.py:86-170), all on bf16x3 products
// (hi*hi + hi*lo + lo*hi, f32 accumulation) of 16x16x32 MFMAs.
#pragma once

#include <cstdint>
#include <vector>

#include "common.h"

namespace wsp {

constexpr int kCamSeg = 100;  // CAMLayer.seg_pooling's segment length

// Weight [N][K] (row stride ldw) -> bf16 hi / lo B fragments of 16x16x32 MFMAs:
// [K/32 k-steps][hi, lo][N/16 column tiles][64 lanes][8]; lane l, element e of k-step ks and
// tile j holds W[16 j + (l & 15)][32 ks + 8 (l >> 4) + e].  K % 32 == 0, N % 16 == 0.
std::vector<uint16_t> cam_pack_b(const float* w, int N, int K, int ldw);

// out[m][n] = epi( sum_k relu(a[m][k] s1[k] + t1[k]) W[n][k] ),  epi(y) = relu(y s2[n] + t2[n])
// or the identity when s2 is null.  The A-side affine + ReLU runs in f32 (one fma) before the
// hi / lo split; s1 null = A as it is (the unfused A/B path).  a = [M][lda] channels-last with
// lda >= K, K % 32 == 0, N % 128 == 0, w = cam_pack_b(W, N, K).
// segsum non-null (N == 128): rows are B = M / T utterances of T frames, a block owns one
// (utterance, 100-frame segment) and also writes the column sums of its output rows,
// segsum[(b * nseg + sg) * N + n] with nseg = ceil(T / 100) — fixed-order f32 tree (lane, then
// the lanes of a column by shuffles, then the four waves in wave order).
struct CamGemmArgs {
  const float* a;
  int lda;
  int M, T, K, N;
  const float* s1;
  const float* t1;
  const void* w;
  const float* s2;
  const float* t2;
  float* out;
  int ldo;
  float* segsum;
};
void launch_cam_gemm(const CamGemmArgs& p, hipStream_t s);

// x[m][k] = relu(x[m][k] s[k] + t[k]) into out [M][ldo] (the unfused pass of the A/B option)
void launch_cam_bnrelu(const float* x, int ldx, int M, int K, const float* sc, const float* sh, float* out, int ldo,
                       hipStream_t s);

// mask[b][sg][n] = sigmoid(b2[n] + sum_j W2[n][j] relu(b1[j] + sum_c W1[j][c] ctx[c])),
// ctx[c] = mean_T(h[b][.][c]) + mean over segment sg of h[b][.][c], from the segment sums of
// launch_cam_gemm (segsum [B][nseg][128]).  w1t = [128][64], w2t = [64][32] (k-major).
void launch_cam_mask(const float* segsum, int B, int T, const float* w1t, const float* b1, const float* w2t,
                     const float* b2, float* mask, hipStream_t s);

// out[m][n] = mask[b][t / 100][n] * sum_{tap < 3, c < 128} h[m + (tap - 1) dil][c] W[n][tap * 128 + c]
// for the 32 output channels n; rows m = b T + t, taps outside the utterance read zero.
// h = [M][ldh], w = cam_pack_b(W [32][384]), out = the 32-column slice [M][ldo] (already offset).
struct CamLocalArgs {
  const float* h;
  int ldh;
  int M, T, dil;
  const void* w;
  const float* mask;
  float* out;
  int ldo;
};
void launch_cam_local(const CamLocalArgs& p, hipStream_t s);

}  // namespace wsp
