// Op-level runner for the CAM++ kernels (tests/test_gpu_campplus_op.py).
//
//   cam_dense_run <case file> <result file>
//
// Reads cases and launches each one through the SHIPPED launchers of libwsp_hip.so
// (launch_cam_gemm, launch_cam_mask, launch_cam_local, launch_fcm_conv) with weights packed by the
// library's own cam_pack_b / pack::conv_kmajor / pack::transpose, then writes back every byte the
// launch could have touched.  It holds no reference arithmetic.
//
// Case file (little-endian): u32 magic 'WSPD' (0x44505357), u32 version (1), u32 ncases, then per
// case u32 op, i32 hdr[8] and the op's arrays, each as u32 count + count f32 values:
//   op 1  BN-ReLU-prologue GEMM   hdr = M, T, K, N, lda, ldo, flags (1: s1 / t1, 2: s2 / t2,
//         4: segment sums), 0     arrays a [M][lda], w [N][K], (s1, t1 [K]), (s2, t2 [N])
//         results out [(M + 8)][ldo], segsum [B nseg N + 128] (empty without flag 4)
//   op 2  context mask            hdr = B, T, 0...
//         arrays segsum [B nseg 128], w1 [64][128], b1 [64], w2 [32][64], b2 [32]
//         results mask [B nseg 32 + 32]
//   op 3  masked local conv       hdr = M, T, dil, ldh, ldo, ocol (first column of the 32-wide
//         slice inside a row of ldo), 0...
//         arrays h [M][ldh], w [32][128][3] (torch layout), mask [B nseg 32]
//         results out [(M + 8)][ldo]
//   op 4  frequency-strided conv  hdr = B, Fi, T, relu, tfc, has_sc, 0...
//         arrays x [B Fi T 32], w [32][32][3][3], bias [32], (wsc [32][32], bsc [32])
//         results out [B Fo T 32 + 256], sc [B Fo T 32 + 256] (empty without has_sc)
// nseg = ceil(T / 100), B = M / T.  Every count is checked against the header: a malformed case
// ends the run with status 2 before anything is launched.
//
// Result file: u32 magic 'WSPR' (0x52505357), u32 ncases, then per case u32 status (0 = ran,
// 1 = refused by a WSP_CHECK), u32 count + message bytes, and when it ran the two result arrays
// (u32 count + f32), pre-filled with the NaN pattern 0x7FC5A5A5: guard rows, guard columns and the
// guard tail must come back untouched.  Any HIP error ends the process with status 3 at once.
#include <hip/hip_runtime.h>

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../wespeaker_hubert_amd/csrc/cam_dense.h"
#include "../wespeaker_hubert_amd/csrc/fcm_conv.h"
#include "../wespeaker_hubert_amd/csrc/pack.h"

using namespace wsp;

namespace {

constexpr uint32_t kMagicIn = 0x44505357u, kMagicOut = 0x52505357u, kVersion = 1, kFill = 0x7FC5A5A5u;
constexpr int kNH = 8;

[[noreturn]] void die(int status, const std::string& msg) {
  std::fprintf(stderr, "cam_dense_run: %s\n", msg.c_str());
  std::fflush(stderr);
  std::exit(status);
}
#define BAD(cond, msg)                                      \
  do {                                                      \
    if (!(cond)) die(2, std::string("bad case: ") + (msg)); \
  } while (0)
#define CK(x)                                                                    \
  do {                                                                           \
    hipError_t e_ = (x);                                                         \
    if (e_ != hipSuccess) die(3, std::string(#x) + ": " + hipGetErrorString(e_)); \
  } while (0)

struct Reader {
  FILE* f;
  void raw(void* dst, size_t n) { BAD(std::fread(dst, 1, n, f) == n, "file too short"); }
  uint32_t u32() {
    uint32_t v;
    raw(&v, 4);
    return v;
  }
  std::vector<float> arr(long long expect, const char* what) {
    const uint32_t n = u32();
    BAD((long long)n == expect, std::string(what) + ": count does not match the header");
    std::vector<float> v(n);
    if (n) raw(v.data(), (size_t)n * 4);
    return v;
  }
};

struct Writer {
  FILE* f;
  void raw(const void* src, size_t n) {
    if (std::fwrite(src, 1, n, f) != n) die(2, "cannot write the result file");
  }
  void u32(uint32_t v) { raw(&v, 4); }
  void arr(const std::vector<float>& v) {
    u32((uint32_t)v.size());
    if (!v.empty()) raw(v.data(), v.size() * 4);
  }
};

struct Pool {
  std::vector<void*> ptrs;
  template <typename T>
  T* up(const std::vector<T>& v) {
    void* d = nullptr;
    CK(hipMalloc(&d, v.empty() ? sizeof(T) : v.size() * sizeof(T)));
    ptrs.push_back(d);
    if (!v.empty()) CK(hipMemcpy(d, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice));
    return static_cast<T*>(d);
  }
  float* filled(size_t n) { return reinterpret_cast<float*>(up(std::vector<uint32_t>(n, kFill))); }
  ~Pool() {
    for (void* d : ptrs) (void)hipFree(d);
  }
};

std::vector<float> down(const float* d, size_t n) {
  std::vector<float> v(n);
  if (n) CK(hipMemcpy(v.data(), d, n * 4, hipMemcpyDeviceToHost));
  return v;
}

void run_case(Reader& in, Writer& out, int index, hipStream_t s) {
  const uint32_t op = in.u32();
  int h[kNH];
  in.raw(h, sizeof(h));
  Pool pool;
  float *d0 = nullptr, *d1 = nullptr;
  size_t n0 = 0, n1 = 0;
  std::string refusal;
  auto guarded = [&](auto&& launch) {
    try {
      launch();
    } catch (const InvalidArg& e) {
      refusal = e.msg;
    } catch (const HipError& e) {
      die(3, e.where + ": " + hipGetErrorString(e.err));
    }
  };
  if (op == 1) {
    const int M = h[0], T = h[1], K = h[2], N = h[3], lda = h[4], ldo = h[5], flags = h[6];
    BAD(M > 0 && M < (1 << 20) && T > 0 && K > 0 && K <= 4096 && N > 0 && N <= 4096, "M / T / K / N out of range");
    BAD(lda >= K && lda <= 8192 && ldo >= N && ldo <= 8192, "lda < K or ldo < N");
    BAD(!(flags & 4) || M % T == 0, "segment sums need M == B * T");
    const std::vector<float> a = in.arr((long long)M * lda, "a"), w = in.arr((long long)N * K, "w");
    std::vector<float> s1, t1, s2, t2;
    if (flags & 1) s1 = in.arr(K, "s1"), t1 = in.arr(K, "t1");
    if (flags & 2) s2 = in.arr(N, "s2"), t2 = in.arr(N, "t2");
    n0 = (size_t)(M + 8) * ldo;
    d0 = pool.filled(n0);
    if (flags & 4) {
      n1 = (size_t)(M / T) * ((T + kCamSeg - 1) / kCamSeg) * N + 128;
      d1 = pool.filled(n1);
    }
    guarded([&] {
      CamGemmArgs p{pool.up(a), lda, M, T, K, N, nullptr, nullptr, pool.up(cam_pack_b(w.data(), N, K, K)),
                    nullptr, nullptr, d0, ldo, d1};
      if (flags & 1) p.s1 = pool.up(s1), p.t1 = pool.up(t1);
      if (flags & 2) p.s2 = pool.up(s2), p.t2 = pool.up(t2);
      launch_cam_gemm(p, s);
    });
  } else if (op == 2) {
    const int B = h[0], T = h[1];
    BAD(B > 0 && B < 4096 && T > 0 && T < (1 << 20), "B / T out of range");
    const int nseg = (T + kCamSeg - 1) / kCamSeg;
    const std::vector<float> ss = in.arr((long long)B * nseg * 128, "segsum"), w1 = in.arr(64 * 128, "w1"),
                             b1 = in.arr(64, "b1"), w2 = in.arr(32 * 64, "w2"), b2 = in.arr(32, "b2");
    n0 = (size_t)B * nseg * 32 + 32;
    d0 = pool.filled(n0);
    guarded([&] {
      launch_cam_mask(pool.up(ss), B, T, pool.up(pack::transpose(w1.data(), 64, 128, 128)), pool.up(b1),
                      pool.up(pack::transpose(w2.data(), 32, 64, 64)), pool.up(b2), d0, s);
    });
  } else if (op == 3) {
    const int M = h[0], T = h[1], dil = h[2], ldh = h[3], ldo = h[4], ocol = h[5];
    BAD(M > 0 && M < (1 << 20) && T > 0 && M % T == 0 && dil >= 1 && dil <= 64, "M / T / dil out of range");
    BAD(ldh >= 128 && ldh <= 8192 && ocol >= 0 && ldo <= 8192 && ocol + 32 <= ldo, "bad strides");
    const int nseg = (T + kCamSeg - 1) / kCamSeg;
    const std::vector<float> hh = in.arr((long long)M * ldh, "h"), w = in.arr(32 * 128 * 3, "w"),
                             mk = in.arr((long long)(M / T) * nseg * 32, "mask");
    n0 = (size_t)(M + 8) * ldo;
    d0 = pool.filled(n0);
    guarded([&] {
      const std::vector<float> wk = pack::conv_kmajor(w, 32, 128, 3, 384);
      const CamLocalArgs p{pool.up(hh), ldh, M, T, dil, pool.up(cam_pack_b(wk.data(), 32, 384, 384)), pool.up(mk),
                           d0 + ocol, ldo};
      launch_cam_local(p, s);
    });
  } else if (op == 4) {
    const int B = h[0], Fi = h[1], T = h[2], relu = h[3], tfc = h[4], has_sc = h[5];
    BAD(B > 0 && Fi > 0 && T > 0 && (long long)B * Fi * T < (1 << 20), "B / Fi / T out of range");
    const int Fo = (Fi - 1) / 2 + 1;
    const std::vector<float> x = in.arr((long long)B * Fi * T * 32, "x"), w = in.arr(32 * 32 * 9, "w"),
                             bias = in.arr(32, "bias");
    std::vector<float> wsc, bsc;
    if (has_sc) wsc = in.arr(32 * 32, "wsc"), bsc = in.arr(32, "bsc");
    n0 = (size_t)B * Fo * T * 32 + 256;
    d0 = pool.filled(n0);
    if (has_sc) {
      n1 = n0;
      d1 = pool.filled(n1);
    }
    guarded([&] {
      const std::vector<float> wk = pack::conv_kmajor(w, 32, 32, 9, 288);
      FcmConvArgs p{pool.up(x), d0, B, Fi, T, pool.up(cam_pack_b(wk.data(), 32, 288, 288)), pool.up(bias), relu, tfc,
                    nullptr, nullptr, nullptr};
      if (has_sc) p.wsc = pool.up(cam_pack_b(wsc.data(), 32, 32, 32)), p.bsc = pool.up(bsc), p.sc = d1;
      launch_fcm_conv(p, s);
    });
  } else {
    BAD(false, "unknown operator");
  }
  CK(hipStreamSynchronize(s));
  CK(hipGetLastError());
  out.u32(refusal.empty() ? 0 : 1);
  out.u32((uint32_t)refusal.size());
  out.raw(refusal.data(), refusal.size());
  if (!refusal.empty()) {
    std::printf("case %d: op %u refused: %s\n", index, op, refusal.c_str());
    return;
  }
  out.arr(down(d0, n0));
  out.arr(down(d1, n1));
  std::printf("case %d: op %u hdr %d %d %d %d %d %d %d\n", index, op, h[0], h[1], h[2], h[3], h[4], h[5], h[6]);
}

}  // namespace

int main(int argc, char** argv) {
  if (argc != 3) die(2, "usage: cam_dense_run <case file> <result file>");
  FILE* fi = std::fopen(argv[1], "rb");
  if (!fi) die(2, std::string("cannot open ") + argv[1]);
  FILE* fo = std::fopen(argv[2], "wb");
  if (!fo) die(2, std::string("cannot open ") + argv[2]);
  Reader in{fi};
  Writer out{fo};
  BAD(in.u32() == kMagicIn, "not a case file");
  BAD(in.u32() == kVersion, "unknown case file version");
  const uint32_t n = in.u32();
  BAD(n >= 1 && n <= 4096, "case count out of range");
  out.u32(kMagicOut);
  out.u32(n);
  hipStream_t s;
  CK(hipStreamCreate(&s));
  for (uint32_t i = 0; i < n; ++i) {
    run_case(in, out, (int)i, s);
    std::fflush(stdout);
  }
  BAD(std::fgetc(fi) == EOF, "trailing bytes after the last case");
  CK(hipStreamDestroy(s));
  std::fclose(fi);
  if (std::fclose(fo) != 0) die(2, "cannot write the result file");
  return 0;
}
