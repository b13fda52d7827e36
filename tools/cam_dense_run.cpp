// Op-level runner for the CAM++ kernels (tests/test_gpu_campplus_op.py).
// Launches launch_cam_gemm, launch_cam_mask, launch_cam_local and launch_fcm_conv of libwsp_hip.so,
// with weights packed by the library's own cam_pack_b / pack::conv_kmajor / pack::transpose.  Framing,
// case and result files: tools/op_runner.h.  Magic 'WSPD' (0x44505357).  Arrays are f32; every op
// sends back two result arrays, the second empty where the op has one.
//
//   op 1  BN-ReLU-prologue GEMM   hdr = M, T, K, N, lda, ldo, flags (1: s1 / t1, 2: s2 / t2,
//         4: segment sums)        arrays a [M][lda], w [N][K], (s1, t1 [K]), (s2, t2 [N])
//         results out [(M + 8)][ldo], segsum [B nseg N + 128] (empty without flag 4)
//   op 2  context mask            hdr = B, T
//         arrays segsum [B nseg 128], w1 [64][128], b1 [64], w2 [32][64], b2 [32]
//         results mask [B nseg 32 + 32]
//   op 3  masked local conv       hdr = M, T, dil, ldh, ldo, ocol (first column of the 32-wide
//         slice inside a row of ldo)
//         arrays h [M][ldh], w [32][128][3] (torch layout), mask [B nseg 32]
//         results out [(M + 8)][ldo]
//   op 4  frequency-strided conv  hdr = B, Fi, T, relu, tfc, has_sc
//         arrays x [B Fi T 32], w [32][32][3][3], bias [32], (wsc [32][32], bsc [32])
//         results out [B Fo T 32 + 256], sc [B Fo T 32 + 256] (empty without has_sc)
// nseg = ceil(T / 100), B = M / T.  Guard rows, guard columns and the guard tail must come back
// untouched.
#include <vector>

#include "../wespeaker_hubert_amd/csrc/cam_dense.h"
#include "../wespeaker_hubert_amd/csrc/fcm_conv.h"
#include "../wespeaker_hubert_amd/csrc/pack.h"
#include "op_runner.h"

using namespace wsp;

namespace {

void run_case(Case& in) {
  const uint32_t op = in.op;
  Pool& pool = in.pool;
  hipStream_t s = in.stream;
  float *d0 = nullptr, *d1 = nullptr;
  size_t n0 = 0, n1 = 0;
  if (op == 1) {
    const int* h = in.h;
    const int M = h[0], T = h[1], K = h[2], N = h[3], lda = h[4], ldo = h[5], flags = h[6];
    BAD(M > 0 && M < (1 << 20) && T > 0 && K > 0 && K <= 4096 && N > 0 && N <= 4096, "M / T / K / N out of range");
    BAD(lda >= K && lda <= 8192 && ldo >= N && ldo <= 8192, "lda < K or ldo < N");
    BAD(!(flags & 4) || M % T == 0, "segment sums need M == B * T");
    const std::vector<float> a = in.f32((long long)M * lda, "a"), w = in.f32((long long)N * K, "w");
    std::vector<float> s1, t1, s2, t2;
    if (flags & 1) s1 = in.f32(K, "s1"), t1 = in.f32(K, "t1");
    if (flags & 2) s2 = in.f32(N, "s2"), t2 = in.f32(N, "t2");
    n0 = (size_t)(M + 8) * ldo;
    d0 = pool.filled(n0);
    if (flags & 4) {
      n1 = (size_t)(M / T) * ((T + kCamSeg - 1) / kCamSeg) * N + 128;
      d1 = pool.filled(n1);
    }
    in.guarded([&] {
      CamGemmArgs p{pool.up(a), lda, M, T, K, N, nullptr, nullptr, pool.up(cam_pack_b(w.data(), N, K, K)),
                    nullptr, nullptr, d0, ldo, d1};
      if (flags & 1) p.s1 = pool.up(s1), p.t1 = pool.up(t1);
      if (flags & 2) p.s2 = pool.up(s2), p.t2 = pool.up(t2);
      launch_cam_gemm(p, s);
    });
  } else if (op == 2) {
    const int* h = in.h;
    const int B = h[0], T = h[1];
    BAD(B > 0 && B < 4096 && T > 0 && T < (1 << 20), "B / T out of range");
    const int nseg = (T + kCamSeg - 1) / kCamSeg;
    const std::vector<float> ss = in.f32((long long)B * nseg * 128, "segsum"), w1 = in.f32(64 * 128, "w1"),
                             b1 = in.f32(64, "b1"), w2 = in.f32(32 * 64, "w2"), b2 = in.f32(32, "b2");
    n0 = (size_t)B * nseg * 32 + 32;
    d0 = pool.filled(n0);
    in.guarded([&] {
      launch_cam_mask(pool.up(ss), B, T, pool.up(pack::transpose(w1.data(), 64, 128, 128)), pool.up(b1),
                      pool.up(pack::transpose(w2.data(), 32, 64, 64)), pool.up(b2), d0, s);
    });
  } else if (op == 3) {
    const int* h = in.h;
    const int M = h[0], T = h[1], dil = h[2], ldh = h[3], ldo = h[4], ocol = h[5];
    BAD(M > 0 && M < (1 << 20) && T > 0 && M % T == 0 && dil >= 1 && dil <= 64, "M / T / dil out of range");
    BAD(ldh >= 128 && ldh <= 8192 && ocol >= 0 && ldo <= 8192 && ocol + 32 <= ldo, "bad strides");
    const int nseg = (T + kCamSeg - 1) / kCamSeg;
    const std::vector<float> hh = in.f32((long long)M * ldh, "h"), w = in.f32(32 * 128 * 3, "w"),
                             mk = in.f32((long long)(M / T) * nseg * 32, "mask");
    n0 = (size_t)(M + 8) * ldo;
    d0 = pool.filled(n0);
    in.guarded([&] {
      const std::vector<float> wk = pack::conv_kmajor(w, 32, 128, 3, 384);
      const CamLocalArgs p{pool.up(hh), ldh, M, T, dil, pool.up(cam_pack_b(wk.data(), 32, 384, 384)), pool.up(mk),
                           d0 + ocol, ldo};
      launch_cam_local(p, s);
    });
  } else if (op == 4) {
    const int* h = in.h;
    const int B = h[0], Fi = h[1], T = h[2], relu = h[3], tfc = h[4], has_sc = h[5];
    BAD(B > 0 && Fi > 0 && T > 0 && (long long)B * Fi * T < (1 << 20), "B / Fi / T out of range");
    const int Fo = (Fi - 1) / 2 + 1;
    const std::vector<float> x = in.f32((long long)B * Fi * T * 32, "x"), w = in.f32(32 * 32 * 9, "w"),
                             bias = in.f32(32, "bias");
    std::vector<float> wsc, bsc;
    if (has_sc) wsc = in.f32(32 * 32, "wsc"), bsc = in.f32(32, "bsc");
    n0 = (size_t)B * Fo * T * 32 + 256;
    d0 = pool.filled(n0);
    if (has_sc) {
      n1 = n0;
      d1 = pool.filled(n1);
    }
    in.guarded([&] {
      const std::vector<float> wk = pack::conv_kmajor(w, 32, 32, 9, 288);
      FcmConvArgs p{pool.up(x), d0, B, Fi, T, pool.up(cam_pack_b(wk.data(), 32, 288, 288)), pool.up(bias), relu, tfc,
                    nullptr, nullptr, nullptr};
      if (has_sc) p.wsc = pool.up(cam_pack_b(wsc.data(), 32, 32, 32)), p.bsc = pool.up(bsc), p.sc = d1;
      launch_fcm_conv(p, s);
    });
  } else {
    BAD(false, "unknown operator");
  }
  in.result(d0, n0);
  in.result(d1, n1);
}

}  // namespace

int main(int argc, char** argv) { return op_runner_main(argc, argv, "cam_dense_run", 0x44505357u, Layout{8, 0, 2}, run_case); }
