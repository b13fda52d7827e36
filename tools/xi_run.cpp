// Op-level runner for XI pooling and the valid-conv offset tables (tests/test_gpu_xi_op.py).
//
//   xi_run <case file> <result file>
//
// Reads cases and launches each one through the SHIPPED launchers of libwsp_hip.so (launch_xi_pool,
// launch_valid_conv_offsets), then writes back every word the launch could have touched.  It holds no
// reference arithmetic.
//
// Case file (little-endian): u32 magic 'WSPX' (0x58505357), u32 version (1), u32 ncases, then per
// case u32 op, i32 hdr[8] and the op's arrays, each as u32 count + count 32-bit words:
//   op 1  XI pooling     hdr = B, T, C, ldz, ldx, ldo, ragged
//         arrays z [rows][ldz] f32, x [rows][ldx] f32, prior_mean [C] f32, prior_logprec [C] f32,
//         seg [B + 1] i32 (ragged; else empty); rows = seg[B] or B T
//         result [B + 2][ldo] f32: the launch gets row 1 as its first output row
//   op 2  offset tables  hdr = B, n, shrink[0..3]
//         arrays off [B + 1] i32
//         result [1 + n (B + 1) + 1] i32: the launch gets word 1 as its first output word
// Every count is checked against the header: a malformed case ends the run with status 2 before
// anything is launched.
//
// Result file: u32 magic 'WSPR' (0x52505357), u32 ncases, then per case u32 status (0 = ran,
// 1 = refused by a WSP_CHECK), u32 count + message bytes, and when it ran the result words
// (u32 count + words), pre-filled with the NaN pattern 0x7FC5A5A5: guard rows, guard words and the
// columns past C must come back untouched.  Any HIP error ends the process with status 3 at once.
#include <hip/hip_runtime.h>

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../wespeaker_hubert_amd/csrc/xi_pool.h"

using namespace wsp;

namespace {

constexpr uint32_t kMagicIn = 0x58505357u, kMagicOut = 0x52505357u, kVersion = 1, kFill = 0x7FC5A5A5u;
constexpr int kNH = 8;

[[noreturn]] void die(int status, const std::string& msg) {
  std::fprintf(stderr, "xi_run: %s\n", msg.c_str());
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
  std::vector<uint32_t> arr(long long expect, const char* what) {
    const uint32_t n = u32();
    BAD((long long)n == expect, std::string(what) + ": count does not match the header");
    std::vector<uint32_t> v(n);
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
  void arr(const std::vector<uint32_t>& v) {
    u32((uint32_t)v.size());
    if (!v.empty()) raw(v.data(), v.size() * 4);
  }
};

struct Pool {
  std::vector<void*> ptrs;
  uint32_t* up(const std::vector<uint32_t>& v) {
    void* d = nullptr;
    CK(hipMalloc(&d, v.empty() ? 4 : v.size() * 4));
    ptrs.push_back(d);
    if (!v.empty()) CK(hipMemcpy(d, v.data(), v.size() * 4, hipMemcpyHostToDevice));
    return static_cast<uint32_t*>(d);
  }
  const float* upf(const std::vector<uint32_t>& v) { return reinterpret_cast<const float*>(up(v)); }
  ~Pool() {
    for (void* d : ptrs) (void)hipFree(d);
  }
};

std::vector<uint32_t> down(const uint32_t* d, size_t n) {
  std::vector<uint32_t> v(n);
  CK(hipDeviceSynchronize());
  CK(hipMemcpy(v.data(), d, n * 4, hipMemcpyDeviceToHost));
  return v;
}

std::vector<uint32_t> run_xi(Reader& r, const int* h) {
  const int B = h[0], T = h[1], C = h[2], ldz = h[3], ldx = h[4], ldo = h[5], ragged = h[6];
  BAD(B >= 1 && B <= 64 && T >= 1 && T <= 4096 && C >= 1 && C <= 4096 && ldz >= C && ldz <= 8192 && ldx >= C &&
          ldx <= 8192 && ldo >= C && ldo <= 8192 && (ragged == 0 || ragged == 1),
      "xi: shape out of range");
  // the arrays follow the header; the segment table comes last, so the row count of a ragged case is
  // read from the array sizes and checked against the table
  const uint32_t nz = r.u32();
  BAD(nz % (uint32_t)ldz == 0 && nz / ldz >= 1 && nz / ldz <= (uint32_t)B * 4096u, "xi: z is not whole rows");
  const long long rows = nz / ldz;
  BAD(ragged || rows == (long long)B * T, "xi: z rows != B T");
  std::vector<uint32_t> z(nz);
  r.raw(z.data(), (size_t)nz * 4);
  const auto x = r.arr(rows * ldx, "x");
  const auto pm = r.arr(C, "prior_mean");
  const auto lp = r.arr(C, "prior_logprec");
  const auto seg = r.arr(ragged ? B + 1 : 0, "seg");
  if (ragged) {
    BAD((int)seg[0] == 0 && (long long)(int)seg[B] == rows, "xi: seg does not span the rows");
    for (int b = 0; b < B; ++b) BAD((int)seg[b + 1] > (int)seg[b], "xi: seg must increase (every utterance >= 1 frame)");
  }
  Pool pool;
  uint32_t* out = pool.up(std::vector<uint32_t>((size_t)(B + 2) * ldo, kFill));
  XiPoolArgs a{pool.upf(z), ldz, pool.upf(x), ldx, pool.upf(pm), pool.upf(lp), B, T, C,
               ragged ? reinterpret_cast<const int*>(pool.up(seg)) : nullptr, reinterpret_cast<float*>(out) + ldo, ldo};
  launch_xi_pool(a, nullptr);
  return down(out, (size_t)(B + 2) * ldo);
}

std::vector<uint32_t> run_offsets(Reader& r, const int* h) {
  const int B = h[0], n = h[1];
  BAD(B >= 1 && B <= 100000 && n >= 1 && n <= 4, "offsets: shape out of range");
  const auto off = r.arr(B + 1, "off");
  Pool pool;
  const size_t words = 2 + (size_t)n * (B + 1);
  uint32_t* out = pool.up(std::vector<uint32_t>(words, kFill));
  launch_valid_conv_offsets(reinterpret_cast<const int*>(pool.up(off)), B, h + 2, n, reinterpret_cast<int*>(out) + 1, nullptr);
  return down(out, words);
}

}  // namespace

int main(int argc, char** argv) {
  if (argc != 3) die(2, "usage: xi_run <case file> <result file>");
  FILE* fi = std::fopen(argv[1], "rb");
  if (!fi) die(2, "cannot open the case file");
  FILE* fo = std::fopen(argv[2], "wb");
  if (!fo) die(2, "cannot open the result file");
  Reader r{fi};
  Writer w{fo};
  BAD(r.u32() == kMagicIn, "magic");
  BAD(r.u32() == kVersion, "version");
  const uint32_t n = r.u32();
  BAD(n <= 4096, "too many cases");
  w.u32(kMagicOut);
  w.u32(n);
  for (uint32_t i = 0; i < n; ++i) {
    const uint32_t op = r.u32();
    int h[kNH];
    r.raw(h, sizeof(h));
    BAD(op == 1 || op == 2, "unknown op");
    std::vector<uint32_t> out;
    std::string msg;
    uint32_t status = 0;
    try {
      out = op == 1 ? run_xi(r, h) : run_offsets(r, h);
    } catch (const InvalidArg& e) {
      status = 1;
      msg = e.msg;
    } catch (const HipError& e) {
      die(3, e.where + ": " + hipGetErrorString(e.err));
    }
    w.u32(status);
    w.u32((uint32_t)msg.size());
    w.raw(msg.data(), msg.size());
    if (status == 0) w.arr(out);
  }
  std::fclose(fi);
  if (std::fclose(fo) != 0) die(2, "cannot write the result file");
  return 0;
}
