// Op-level runner for XI pooling and the valid-conv offset tables (tests/test_gpu_xi_op.py).
// Launches launch_xi_pool and launch_valid_conv_offsets of libwsp_hip.so.  Framing, case and result
// files: tools/op_runner.h.  Magic 'WSPX' (0x58505357).
//
//   op 1  XI pooling     hdr = B, T, C, ldz, ldx, ldo, ragged
//         arrays z [rows][ldz] f32, x [rows][ldx] f32, prior_mean [C] f32, prior_logprec [C] f32,
//         seg [B + 1] i32 (ragged; else empty); rows = seg[B] or B T
//         result [B + 2][ldo] f32: the launch gets row 1 as its first output row
//   op 2  offset tables  hdr = B, n, shrink[0..3]
//         arrays off [B + 1] i32
//         result [1 + n (B + 1) + 1] i32: the launch gets word 1 as its first output word
// Guard rows, guard words and the columns past C must come back untouched.
#include <vector>

#include "../wespeaker_hubert_amd/csrc/xi_pool.h"
#include "op_runner.h"

using namespace wsp;

namespace {

void run_xi(Case& c) {
  const int* h = c.h;
  const int B = h[0], T = h[1], C = h[2], ldz = h[3], ldx = h[4], ldo = h[5], ragged = h[6];
  BAD(B >= 1 && B <= 64 && T >= 1 && T <= 4096 && C >= 1 && C <= 4096 && ldz >= C && ldz <= 8192 && ldx >= C &&
          ldx <= 8192 && ldo >= C && ldo <= 8192 && (ragged == 0 || ragged == 1),
      "xi: shape out of range");
  // the segment table comes last, so the row count of a ragged case is read from the array sizes and
  // checked against the table
  const uint32_t nz = c.next_count();
  BAD(nz % (uint32_t)ldz == 0 && nz / ldz >= 1 && nz / ldz <= (uint32_t)B * 4096u, "xi: z is not whole rows");
  const long long rows = nz / ldz;
  BAD(ragged || rows == (long long)B * T, "xi: z rows != B T");
  const auto z = c.f32(nz, "z");
  const auto x = c.f32(rows * ldx, "x");
  const auto pm = c.f32(C, "prior_mean");
  const auto lp = c.f32(C, "prior_logprec");
  const auto seg = c.i32(ragged ? B + 1 : 0, "seg");
  if (ragged) {
    BAD(seg[0] == 0 && (long long)seg[B] == rows, "xi: seg does not span the rows");
    for (int b = 0; b < B; ++b) BAD(seg[b + 1] > seg[b], "xi: seg must increase (every utterance >= 1 frame)");
  }
  Pool& pool = c.pool;
  float* out = pool.filled((size_t)(B + 2) * ldo);
  c.result(out, (size_t)(B + 2) * ldo);
  c.guarded([&] {
    XiPoolArgs a{pool.up(z), ldz, pool.up(x), ldx, pool.up(pm), pool.up(lp), B, T, C,
                 ragged ? pool.up(seg) : nullptr, out + ldo, ldo};
    launch_xi_pool(a, c.stream);
  });
}

void run_offsets(Case& c) {
  const int* h = c.h;
  const int B = h[0], n = h[1];
  BAD(B >= 1 && B <= 100000 && n >= 1 && n <= 4, "offsets: shape out of range");
  const auto off = c.i32(B + 1, "off");
  Pool& pool = c.pool;
  const size_t words = 2 + (size_t)n * (B + 1);
  float* out = pool.filled(words);
  c.result(out, words);
  c.guarded([&] { launch_valid_conv_offsets(pool.up(off), B, h + 2, n, reinterpret_cast<int*>(out) + 1, c.stream); });
}

void run_case(Case& c) {
  BAD(c.op == 1 || c.op == 2, "unknown operator");
  c.op == 1 ? run_xi(c) : run_offsets(c);
}

}  // namespace

int main(int argc, char** argv) { return op_runner_main(argc, argv, "xi_run", 0x58505357u, Layout{8, 0, 1}, run_case); }
