// Op-level runner for the ERes2Net kernels (tests/test_gpu_eres2net_op.py).
//
//   eres2net_run <case file> <result file>
//
// Reads cases and launches each one through the SHIPPED launchers of libwsp_hip.so
// (launch_eres_conv3x3, launch_eres_pw, launch_eres_aff) with weights packed by the library's own
// pack::frag16 / pack::conv_kmajor, then writes back every byte the launch could have touched.  It
// holds no reference arithmetic.
//
// Case file (little-endian): u32 magic 'WSPE' (0x45505357), u32 version (1), u32 ncases, then per
// case u32 op, i32 hdr[16] and the op's arrays, each as u32 count + count f32 values:
//   op 1  conv (3x3 Res2 step / 1x1)   hdr = taps (9 or 1), B, Fi, Ti, cin, N, stride, lda, aoff,
//         a2off (-1: no added slice), ldo, ooff, act, has_res, 0, 0
//         arrays a [B Fi Ti][lda], (a2 [B Fi Ti][lda]), w [N][cin][taps] (torch layout), bias [N],
//         (res [M][N]);  the slices read start at channel aoff / a2off of a row, the slice written at
//         channel ooff of a row of ldo;  results out [(M + 8)][ldo],  M = B Fo To
//   op 2  AFF                          hdr = M, C, ldx, xoff, ldy, yoff, ldo, ooff, 0...
//         arrays x [M][ldx], y [M][ldy], wa [C/4][2C], ba [C/4], wb [C][C/4], bb [C]
//         results out [(M + 8)][ldo]
// Every count is checked against the header: a malformed case ends the run with status 2 before
// anything is launched.
//
// Result file: u32 magic 'WSPR' (0x52505357), u32 ncases, then per case u32 status (0 = ran,
// 1 = refused by a WSP_CHECK), u32 count + message bytes, and when it ran the result array
// (u32 count + f32), pre-filled with the NaN pattern 0x7FC5A5A5: guard rows and guard columns must
// come back untouched.  Any HIP error ends the process with status 3 at once.
#include <hip/hip_runtime.h>

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../wespeaker_hubert_amd/csrc/eres2net.h"
#include "../wespeaker_hubert_amd/csrc/pack.h"

using namespace wsp;

namespace {

constexpr uint32_t kMagicIn = 0x45505357u, kMagicOut = 0x52505357u, kVersion = 1, kFill = 0x7FC5A5A5u;
constexpr int kNH = 16;

[[noreturn]] void die(int status, const std::string& msg) {
  std::fprintf(stderr, "eres2net_run: %s\n", msg.c_str());
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
  float* d0 = nullptr;
  size_t n0 = 0;
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
    const int taps = h[0], B = h[1], Fi = h[2], Ti = h[3], cin = h[4], N = h[5], stride = h[6], lda = h[7], aoff = h[8],
              a2off = h[9], ldo = h[10], ooff = h[11], act = h[12], has_res = h[13];
    BAD((taps == 1 || taps == 9) && B > 0 && Fi > 0 && Ti > 0 && (long long)B * Fi * Ti < (1 << 20), "shape out of range");
    BAD(cin > 0 && cin <= 4096 && N > 0 && N <= 4096 && (stride == 1 || stride == 2), "cin / N / stride out of range");
    BAD(aoff >= 0 && aoff + cin <= lda && lda <= 8192 && a2off >= -1 && a2off + cin <= lda, "bad input slice");
    BAD(ooff >= 0 && ooff + N <= ldo && ldo <= 8192, "bad output slice");
    const long long rows = (long long)B * Fi * Ti;
    const int Fo = (Fi - 1) / stride + 1, To = (Ti - 1) / stride + 1, M = B * Fo * To;
    const std::vector<float> a = in.arr(rows * lda, "a");
    std::vector<float> a2, res;
    if (a2off >= 0) a2 = in.arr(rows * lda, "a2");
    const std::vector<float> w = in.arr((long long)N * cin * taps, "w"), bias = in.arr(N, "bias");
    if (has_res) res = in.arr((long long)M * N, "res");
    n0 = (size_t)(M + 8) * ldo;
    d0 = pool.filled(n0);
    guarded([&] {
      const int K = cin * taps;
      const std::vector<float> wk = pack::conv_kmajor(w, N, cin, taps, K);
      EresConvArgs p{pool.up(a) + aoff, lda, nullptr, 0,   B,   Fi,   Ti, cin, stride, pool.up(pack::frag16(wk.data(), N, K, K)),
                     pool.up(bias),     N,   nullptr, 0,   d0 + ooff, ldo, act};
      if (a2off >= 0) p.a2 = pool.up(a2) + a2off, p.lda2 = lda;
      if (has_res) p.res = pool.up(res), p.ldres = N;
      if (taps == 9)
        launch_eres_conv3x3(p, s);
      else
        launch_eres_pw(p, s);
    });
  } else if (op == 2) {
    const int M = h[0], C = h[1], ldx = h[2], xoff = h[3], ldy = h[4], yoff = h[5], ldo = h[6], ooff = h[7];
    BAD(M > 0 && M < (1 << 20) && C >= 4 && C <= 4096 && C % 4 == 0, "M / C out of range");
    BAD(xoff >= 0 && xoff + C <= ldx && ldx <= 8192 && yoff >= 0 && yoff + C <= ldy && ldy <= 8192, "bad input slices");
    BAD(ooff >= 0 && ooff + C <= ldo && ldo <= 8192, "bad output slice");
    const int H = C / 4, Hp = (H + 31) / 32 * 32;
    const std::vector<float> x = in.arr((long long)M * ldx, "x"), y = in.arr((long long)M * ldy, "y"),
                             wa = in.arr((long long)H * 2 * C, "wa"), ba = in.arr(H, "ba"),
                             wb = in.arr((long long)C * H, "wb"), bb = in.arr(C, "bb");
    n0 = (size_t)(M + 8) * ldo;
    d0 = pool.filled(n0);
    guarded([&] {
      // rows / columns [H, Hp) zero, as the model's fold_aff lays them out
      std::vector<float> wap((size_t)Hp * 2 * C, 0.f), bap(Hp, 0.f), wbp((size_t)C * Hp, 0.f);
      std::copy(wa.begin(), wa.end(), wap.begin());
      std::copy(ba.begin(), ba.end(), bap.begin());
      for (int n = 0; n < C; ++n) std::copy(wb.begin() + (size_t)n * H, wb.begin() + (size_t)(n + 1) * H, wbp.begin() + (size_t)n * Hp);
      const EresAffArgs p{pool.up(x) + xoff, ldx, pool.up(y) + yoff, ldy, M, C,
                          pool.up(pack::frag16(wap.data(), Hp, 2 * C, 2 * C)), pool.up(bap),
                          pool.up(pack::frag16(wbp.data(), C, Hp, Hp, true)), pool.up(bb), d0 + ooff, ldo};
      launch_eres_aff(p, s);
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
  std::printf("case %d: op %u hdr %d %d %d %d %d %d %d %d\n", index, op, h[0], h[1], h[2], h[3], h[4], h[5], h[6], h[7]);
}

}  // namespace

int main(int argc, char** argv) {
  if (argc != 3) die(2, "usage: eres2net_run <case file> <result file>");
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
