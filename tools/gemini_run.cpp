// Op-level runner for the Gemini DF-ResNet kernels (tests/test_gpu_gemini_op.py).
//
//   gemini_run <case file> <result file>
//
// Reads cases and launches each one through the SHIPPED launchers of libwsp_hip.so
// (launch_gemini_dw, launch_gemini_tail, launch_gemini_down and, for the bottleneck's 1x1 convs,
// launch_conv_gemm_x3 with the family's tile family 7) with weights packed by the library's own
// pack::frag16 / pack::conv_kmajor / pack::split, then writes back every byte the launch could have
// touched.  It holds no reference arithmetic.
//
// Case file (little-endian): u32 magic 'WSPG' (0x47505357), u32 version (1), u32 ncases, then per
// case u32 op, i32 hdr[16] and the op's arrays, each as u32 count + count f32 values:
//   op 1  depthwise 3x3     hdr = B, F, T, C, ldy, yoff, ldo, ooff
//         arrays y [B F T][ldy], w [9][C] (tap-major), b [C]
//   op 2  bottleneck tail   hdr = B, F, T, d, ldy, yoff, ldres, roff, ldo, ooff        (K = 4 d)
//         arrays y1 [B F T][ldy], w2 [9][K], b2 [K], w3 [d][K], b3 [d], res [B F T][ldres]
//   op 3  downsample 3x3    hdr = B, Fi, Ti, cin, N, sf, st, lda, aoff, ldo, ooff
//         arrays a [B Fi Ti][lda], w [N][cin][9] (torch layout), bias [N]
//   op 4  1x1 conv + ReLU   hdr = M, cin, N, has_res, lda, aoff, ldo, ooff
//         arrays a [M][lda], w [N][cin], bias [N], (res [M][N])
// The slices read start at channel yoff / aoff / roff of a row, the slice written at channel ooff
// of a row of ldo; results out [(M + 8)][ldo], M = the output positions.  Every count is checked
// against the header: a malformed case ends the run with status 2 before anything is launched.
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

#include "../wespeaker_hubert_amd/csrc/gemini.h"
#include "../wespeaker_hubert_amd/csrc/kernels.h"
#include "../wespeaker_hubert_amd/csrc/pack.h"

using namespace wsp;

namespace {

constexpr uint32_t kMagicIn = 0x47505357u, kMagicOut = 0x52505357u, kVersion = 1, kFill = 0x7FC5A5A5u;
constexpr int kNH = 16;
constexpr int kX3Variant = 7;  // the family's tile family (make_gemini)

[[noreturn]] void die(int status, const std::string& msg) {
  std::fprintf(stderr, "gemini_run: %s\n", msg.c_str());
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

bool slice_ok(int off, int width, int ld) { return off >= 0 && width > 0 && off + width <= ld && ld <= 8192; }

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
  auto plane_ok = [](int B, int F, int T) { return B > 0 && F > 0 && T > 0 && (long long)B * F * T < (1 << 20); };
  if (op == 1) {
    const int B = h[0], F = h[1], T = h[2], C = h[3], ldy = h[4], yoff = h[5], ldo = h[6], ooff = h[7];
    BAD(plane_ok(B, F, T) && C > 0 && C <= 4096, "shape out of range");
    BAD(slice_ok(yoff, C, ldy) && slice_ok(ooff, C, ldo), "bad slices");
    const long long M = (long long)B * F * T;
    const std::vector<float> y = in.arr(M * ldy, "y"), w = in.arr(9LL * C, "w"), b = in.arr(C, "b");
    n0 = (size_t)(M + 8) * ldo;
    d0 = pool.filled(n0);
    guarded([&] {
      const GeminiDwArgs p{pool.up(y) + yoff, ldy, B, F, T, C, pool.up(w), pool.up(b), d0 + ooff, ldo};
      launch_gemini_dw(p, s);
    });
  } else if (op == 2) {
    const int B = h[0], F = h[1], T = h[2], d = h[3], ldy = h[4], yoff = h[5], ldres = h[6], roff = h[7], ldo = h[8],
              ooff = h[9];
    BAD(plane_ok(B, F, T) && d > 0 && d <= 1024, "shape out of range");
    const int K = 4 * d;
    BAD(slice_ok(yoff, K, ldy) && slice_ok(roff, d, ldres) && slice_ok(ooff, d, ldo), "bad slices");
    const long long M = (long long)B * F * T;
    const std::vector<float> y1 = in.arr(M * ldy, "y1"), w2 = in.arr(9LL * K, "w2"), b2 = in.arr(K, "b2"),
                             w3 = in.arr((long long)d * K, "w3"), b3 = in.arr(d, "b3"), res = in.arr(M * ldres, "res");
    n0 = (size_t)(M + 8) * ldo;
    d0 = pool.filled(n0);
    guarded([&] {
      const GeminiTailArgs p{pool.up(y1) + yoff, ldy,         B,           F,
                             T,                  d,           pool.up(w2), pool.up(b2),
                             pool.up(pack::frag16(w3.data(), d, K, K)),    pool.up(b3),
                             pool.up(res) + roff, ldres,      d0 + ooff,   ldo};
      launch_gemini_tail(p, s);
    });
  } else if (op == 3) {
    const int B = h[0], Fi = h[1], Ti = h[2], cin = h[3], N = h[4], sf = h[5], st = h[6], lda = h[7], aoff = h[8],
              ldo = h[9], ooff = h[10];
    BAD(plane_ok(B, Fi, Ti) && cin > 0 && cin <= 1024 && N > 0 && N <= 1024 && sf >= 1 && sf <= 4 && st >= 1 && st <= 4,
        "shape out of range");
    BAD(slice_ok(aoff, cin, lda) && slice_ok(ooff, N, ldo), "bad slices");
    const long long rows = (long long)B * Fi * Ti;
    const int Fo = (Fi - 1) / sf + 1, To = (Ti - 1) / st + 1, M = B * Fo * To;
    const std::vector<float> a = in.arr(rows * lda, "a"), w = in.arr((long long)N * cin * 9, "w"), bias = in.arr(N, "bias");
    n0 = (size_t)(M + 8) * ldo;
    d0 = pool.filled(n0);
    guarded([&] {
      const int K = 9 * cin;
      const std::vector<float> wk = pack::conv_kmajor(w, N, cin, 9, K);
      const GeminiDownArgs p{pool.up(a) + aoff, lda, B, Fi, Ti, cin, sf, st, pool.up(pack::frag16(wk.data(), N, K, K)),
                             pool.up(bias),     N,   d0 + ooff, ldo};
      launch_gemini_down(p, s);
    });
  } else if (op == 4) {
    const int M = h[0], cin = h[1], N = h[2], has_res = h[3], lda = h[4], aoff = h[5], ldo = h[6], ooff = h[7];
    BAD(M > 0 && M < (1 << 20) && cin > 0 && cin <= 4096 && N > 0 && N <= 4096, "shape out of range");
    BAD(slice_ok(aoff, cin, lda) && slice_ok(ooff, N, ldo), "bad slices");
    const std::vector<float> a = in.arr((long long)M * lda, "a"), w = in.arr((long long)N * cin, "w"), bias = in.arr(N, "bias");
    std::vector<float> res;
    if (has_res) res = in.arr((long long)M * N, "res");
    n0 = (size_t)(M + 8) * ldo;
    d0 = pool.filled(n0);
    guarded([&] {
      // as Gemini::forward fills it (Impl::one_operand / fill): one dense segment, one "utterance" of M rows
      const int Kp = (cin + 63) / 64 * 64;
      std::vector<uint16_t> whi, wlo;
      pack::split(pack::conv_kmajor(w, N, cin, 1, Kp), whi, wlo);
      ConvGemmArgs g{};
      const float* da = pool.up(a) + aoff;
      g.a[0] = g.a[1] = g.a[2] = da;
      g.lda[0] = g.lda[1] = g.lda[2] = lda;
      g.cseg[1] = g.cseg[2] = g.cseg[3] = cin;
      g.cin = cin, g.taps = 1, g.dil = 1, g.pad = 0;
      g.M = M, g.T = M, g.N = N, g.K = cin, g.Kp = Kp;
      g.bias = pool.up(bias);
      g.out = d0 + ooff, g.ldo = ldo, g.act = kActRelu;
      if (has_res) g.res = pool.up(res), g.ldres = N, g.role = 2;
      launch_conv_gemm_x3(g, pool.up(whi), pool.up(wlo), kX3Variant, s);
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
  if (argc != 3) die(2, "usage: gemini_run <case file> <result file>");
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
