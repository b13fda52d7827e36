// The framing every op-level runner shares (tools/*_run.cpp; the Python side is tests/op_runner.py).
//
//   <runner> <case file> <result file>
//
// A runner reads cases, launches each one through the SHIPPED launchers of libwsp_hip.so and sends
// back every word the launch could have touched.  It holds no reference arithmetic.  What a runner
// adds to this file is its magic, its Layout and its op table: the header ints, arrays and results
// of each op.
//
// Case file, version 1 (little-endian, 32-bit words throughout):
//   u32 magic (the runner's own), u32 version = 1, u32 ncases (1 .. 4096), then per case
//   u32 op, Layout::nh x i32 header (fields an op does not use are 0), then the op's arrays, each as
//   u32 count + count words (f32 or i32, as the op table says).
// The runner takes the arrays in order (Case::f32 / i32), each with the count the header implies;
// optional arrays are decided by the header.  A short file, a count that does not match or bytes after
// the last case end the run with status 2 before that case launches anything.
//
// Result file:
//   u32 magic 'WSPR' (0x52505357), u32 ncases, then per case
//   u32 status (0 = ran, 1 = refused by a WSP_CHECK of the library), Layout::own words of the runner's
//   own (Case::own; written for refused cases too), u32 n + n message bytes (the refusal), and, when it
//   ran, the result arrays, each as u32 count + count words: Layout::narrays of them, or, where that
//   is 0, u32 narrays first.
// Result buffers come from Pool::filled, pre-filled with the NaN pattern 0x7FC5A5A5: guard rows,
// guard columns and guard words must come back untouched.
//
// One line per case goes to stdout.  Any HIP error ends the process with status 3 at once.  A run that
// ends with a status other than 0 leaves an empty result file.
#pragma once
#include <hip/hip_runtime.h>
#include <unistd.h>

#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <utility>
#include <vector>

#include "../wespeaker_hubert_amd/csrc/common.h"

namespace op_runner {

constexpr uint32_t kMagicOut = 0x52505357u, kVersion = 1, kFill = 0x7FC5A5A5u;
constexpr uint32_t kMaxCases = 4096;
constexpr int kMaxHdr = 64, kMaxOwn = 8;

// what differs between the runners' files
struct Layout {
  int nh;       // header ints of a case
  int own;      // words of the runner's own after a result's status
  int narrays;  // result arrays of a case that ran; 0: their number is written in front of them
};

inline const char* g_name = "op_runner";  // both set by op_runner_main
inline FILE* g_result = nullptr;

// A run that dies leaves an empty result file: no reader can take the cases before the fault for a whole run.
[[noreturn]] inline void die(int status, const std::string& msg) {
  std::fprintf(stderr, "%s: %s\n", g_name, msg.c_str());
  std::fflush(stderr);
  if (g_result && (std::fflush(g_result) != 0 || ftruncate(fileno(g_result), 0) != 0))
    std::fprintf(stderr, "%s: cannot empty the result file\n", g_name);
  std::exit(status);
}
#define BAD(cond, msg)                                                  \
  do {                                                                  \
    if (!(cond)) op_runner::die(2, std::string("bad case: ") + (msg));  \
  } while (0)
#define CK(x)                                                                                \
  do {                                                                                       \
    hipError_t e_ = (x);                                                                     \
    if (e_ != hipSuccess) op_runner::die(3, std::string(#x) + ": " + hipGetErrorString(e_)); \
  } while (0)

struct Reader {
  FILE* f;
  size_t left;  // bytes of the file not read yet: a count past the end fails before anything is allocated
  explicit Reader(FILE* file) : f(file), left(0) {
    BAD(std::fseek(f, 0, SEEK_END) == 0 && std::ftell(f) >= 0, "cannot size the case file");
    left = (size_t)std::ftell(f);
    std::rewind(f);
  }
  void raw(void* dst, size_t n) {
    BAD(n <= left && std::fread(dst, 1, n, f) == n, "file too short");
    left -= n;
  }
  uint32_t u32() {
    uint32_t v;
    raw(&v, 4);
    return v;
  }
};

struct Writer {
  FILE* f;
  void raw(const void* src, size_t n) {
    if (n && std::fwrite(src, 1, n, f) != n) die(2, "cannot write the result file");
  }
  void u32(uint32_t v) { raw(&v, 4); }
  void text(const std::string& s) {
    u32((uint32_t)s.size());
    raw(s.data(), s.size());
  }
  void arr(const std::vector<uint32_t>& v) {
    u32((uint32_t)v.size());
    raw(v.data(), v.size() * 4);
  }
};

// device buffers of one case
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
  Pool() = default;
  Pool(const Pool&) = delete;
  Pool& operator=(const Pool&) = delete;
  ~Pool() {
    for (void* d : ptrs) (void)hipFree(d);
  }
};

inline std::vector<uint32_t> down(const void* d, size_t n) {
  std::vector<uint32_t> v(n);
  if (n) CK(hipMemcpy(v.data(), d, n * 4, hipMemcpyDeviceToHost));
  return v;
}

// One case: what the file says, the stream to launch on, and what goes back.
struct Case {
  int index = 0;
  uint32_t op = 0;
  int h[kMaxHdr] = {};  // the header ints (Layout::nh of them)
  hipStream_t stream = nullptr;
  Pool pool;
  uint32_t own[kMaxOwn] = {};  // the runner's own words of the result record (Layout::own of them)
  std::string note;            // free text for the stdout line

  // the next array of the file, which must hold `expect` values
  std::vector<float> f32(long long expect, const char* what) { return take<float>(expect, what); }
  std::vector<int> i32(long long expect, const char* what) { return take<int>(expect, what); }
  // the count of the next array, where the header alone does not give it
  uint32_t next_count() {
    if (!peeked_) count_ = in_->u32();
    peeked_ = true;
    return count_;
  }
  // `n` words at device pointer `d` go back as the next result array, read after the stream has drained
  void result(const void* d, size_t n) { results_.emplace_back(d, n); }
  // runs the launch: a WSP_CHECK of the library refuses the case, anything else thrown is fatal
  template <typename F>
  void guarded(F&& launch) {
    try {
      launch();
    } catch (const wsp::InvalidArg& e) {
      refused_ = true;
      message_ = e.msg;
    } catch (const wsp::HipError& e) {
      die(3, e.where + ": " + hipGetErrorString(e.err));
    } catch (...) {
      die(3, "unknown exception from the library");
    }
  }

 private:
  friend int op_runner_main(int, char**, const char*, uint32_t, const Layout&, void (*)(Case&));
  template <typename T>
  std::vector<T> take(long long expect, const char* what) {
    static_assert(sizeof(T) == 4, "32-bit words");
    const uint32_t n = next_count();
    peeked_ = false;
    BAD((long long)n == expect, std::string(what) + ": count does not match the header");
    BAD((size_t)n * 4 <= in_->left, "file too short");
    std::vector<T> v(n);
    if (n) in_->raw(v.data(), (size_t)n * 4);
    return v;
  }
  Reader* in_ = nullptr;
  bool peeked_ = false;
  uint32_t count_ = 0;
  std::vector<std::pair<const void*, size_t>> results_;
  bool refused_ = false;
  std::string message_;
};

inline int op_runner_main(int argc, char** argv, const char* name, uint32_t magic, const Layout& lay,
                          void (*fn)(Case&)) {
  g_name = name;
  if (argc != 3) die(2, std::string("usage: ") + name + " <case file> <result file>");
  FILE* fi = std::fopen(argv[1], "rb");
  if (!fi) die(2, std::string("cannot open ") + argv[1]);
  FILE* fo = std::fopen(argv[2], "wb");
  if (!fo) die(2, std::string("cannot open ") + argv[2]);
  g_result = fo;
  Reader in(fi);
  Writer out{fo};
  BAD(in.u32() == magic, "not a case file of this runner (magic)");
  BAD(in.u32() == kVersion, "unknown case file version");
  const uint32_t n = in.u32();
  BAD(n >= 1 && n <= kMaxCases, "case count out of range");
  out.u32(kMagicOut);
  out.u32(n);
  hipStream_t s;
  CK(hipStreamCreate(&s));
  for (uint32_t i = 0; i < n; ++i) {
    Case c;
    c.index = (int)i;
    c.stream = s;
    c.in_ = &in;
    c.op = in.u32();
    in.raw(c.h, (size_t)lay.nh * 4);
    fn(c);
    CK(hipStreamSynchronize(s));
    CK(hipGetLastError());
    out.u32(c.refused_ ? 1 : 0);
    out.raw(c.own, (size_t)lay.own * 4);
    out.text(c.message_);
    std::printf("case %d: op %u", c.index, c.op);
    if (c.refused_) {
      std::printf(" refused: %s", c.message_.c_str());
    } else {
      if (!lay.narrays)
        out.u32((uint32_t)c.results_.size());
      else if ((int)c.results_.size() != lay.narrays)
        die(3, "the runner sends another number of result arrays than its layout says");
      for (const auto& r : c.results_) out.arr(down(r.first, r.second));
      std::printf(" hdr");
      for (int k = 0; k < lay.nh && k < 8; ++k) std::printf(" %d", c.h[k]);
    }
    std::printf("%s%s\n", c.note.empty() ? "" : "  ", c.note.c_str());
    std::fflush(stdout);
  }
  BAD(in.left == 0, "trailing bytes after the last case");
  CK(hipStreamDestroy(s));
  std::fclose(fi);
  g_result = nullptr;
  if (std::fclose(fo) != 0) die(2, "cannot write the result file");
  return 0;
}

}  // namespace op_runner

using op_runner::Case;
using op_runner::Layout;
using op_runner::op_runner_main;
using op_runner::Pool;
