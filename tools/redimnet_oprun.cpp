// Op-level runner for the ReDimNet kernels (tests/test_gpu_redimnet_op.py): launches the shipped
// launchers of redimnet.h in libwsp_hip.so.  Framing, case and result files: tools/op_runner.h.
// Magic 'WSPD' (0x44505357).  Arrays are f32; one result array per case.
//
//   op 1  stem            hdr = B, T, ldo                 arrays feats [B T][72], w [9][16], bias, gamma, beta [16]
//   op 2  stage entry     hdr = rows, n, gw, ld_in, ldo   arrays in [n][rows][ld_in], sw [n][1152], (wt [gw][gw], bias [gw])
//   op 3  2-D block       hdr = B, T, F, c, ldx, ldo      arrays x [B T][ldx], wd [36][c], bd [c], wp [c][c], bp [c]
//   op 4  1-D block       hdr = B, T, C, k, ldx, ldo      arrays x [B T][ldx], wd [k][C], bd [C], wp [C][C], bp [C]
//   op 5  LayerNorm       hdr = M, D, has_add, ldx, ldadd, ldo   arrays x [M][ldx], (add [M][ldadd]), gamma, beta [D]
//   op 6  attention       hdr = B, T, H, dh, ld, ldo      arrays qkv [B T][ld]                 (scale = dh^-0.5)
//   op 7  NewGELU         hdr = M, D, ldx                 arrays x [M][ldx]                    (in place)
// Weights travel in the kernels' own order (tap-major / k-major, redimnet.h); LayerNorm eps is 1e-6.
// Results: out [(rows + 8)][ldo] pre-filled with the guard pattern (op 7: the [M][ldx] buffer itself,
// whose pad columns must come back as they went in).
#include <cmath>
#include <vector>

#include "../wespeaker_hubert_amd/csrc/redimnet.h"
#include "op_runner.h"

using namespace wsp;

namespace {

bool ld_ok(int width, int ld) { return width > 0 && ld >= width && ld <= 8192; }

void run_case(Case& in) {
  const uint32_t op = in.op;
  const int* h = in.h;
  Pool& pool = in.pool;
  hipStream_t s = in.stream;
  float* d0 = nullptr;
  size_t n0 = 0;
  auto rows_ok = [](long long B, long long T) { return B > 0 && T > 0 && B * T < (1 << 16); };
  if (op == 1) {
    const int B = h[0], T = h[1], ldo = h[2];
    BAD(rows_ok(B, T) && ld_ok(kRdWidth, ldo), "shape out of range");
    const long long M = (long long)B * T;
    const std::vector<float> x = in.f32(M * 72, "feats"), w = in.f32(144, "w"), b = in.f32(16, "bias"),
                             g = in.f32(16, "gamma"), be = in.f32(16, "beta");
    n0 = (size_t)(M + 8) * ldo;
    d0 = pool.filled(n0);
    in.guarded([&] { launch_rd_stem({pool.up(x), B, T, 72, pool.up(w), pool.up(b), pool.up(g), pool.up(be), 1e-6f, d0, ldo}, s); });
  } else if (op == 2) {
    const int rows = h[0], n = h[1], gw = h[2], ld_in = h[3], ldo = h[4];
    BAD(rows_ok(rows, 1) && n >= 1 && n <= kRdMaxIn && gw >= 0 && gw <= 1152 && ld_ok(kRdWidth, ld_in) && ld_ok(kRdWidth, ldo),
        "shape out of range");
    const std::vector<float> x = in.f32((long long)n * rows * ld_in, "in"), sw = in.f32((long long)n * kRdWidth, "sw");
    std::vector<float> wt, b;
    if (gw) wt = in.f32((long long)gw * gw, "wt"), b = in.f32(gw, "bias");
    n0 = (size_t)(rows + 8) * ldo;
    d0 = pool.filled(n0);
    in.guarded([&] {
      RdEntryArgs p{};
      const float* dx = pool.up(x);
      for (int i = 0; i < n; ++i) p.in[i] = dx + (size_t)i * rows * ld_in;
      p.ld_in = ld_in, p.n = n, p.sw = pool.up(sw), p.rows = rows, p.gw = gw;
      p.wt = gw ? pool.up(wt) : nullptr, p.bias = gw ? pool.up(b) : nullptr, p.out = d0, p.ldo = ldo;
      launch_rd_entry(p, s);
    });
  } else if (op == 3 || op == 4) {
    const int B = h[0], T = h[1], a2 = h[2], a3 = h[3], ldx = h[4], ldo = h[5];
    const int C = op == 3 ? a3 : a2, width = op == 3 ? kRdWidth : C, taps = op == 3 ? 36 : a3;
    BAD(rows_ok(B, T) && a2 > 0 && a2 <= 1152 && a3 > 0 && a3 <= 1152 && ld_ok(width, ldx) && ld_ok(width, ldo),
        "shape out of range");
    const long long M = (long long)B * T;
    const std::vector<float> x = in.f32(M * ldx, "x"), wd = in.f32((long long)taps * C, "wd"), bd = in.f32(C, "bd"),
                             wp = in.f32((long long)C * C, "wp"), bp = in.f32(C, "bp");
    n0 = (size_t)(M + 8) * ldo;
    d0 = pool.filled(n0);
    in.guarded([&] {
      if (op == 3)
        launch_rd_block2d({pool.up(x), ldx, B, T, a2, a3, pool.up(wd), pool.up(bd), pool.up(wp), pool.up(bp), d0, ldo}, s);
      else
        launch_rd_block1d({pool.up(x), ldx, B, T, a2, a3, pool.up(wd), pool.up(bd), pool.up(wp), pool.up(bp), d0, ldo}, s);
    });
  } else if (op == 5) {
    const int M = h[0], D = h[1], has_add = h[2], ldx = h[3], ldadd = h[4], ldo = h[5];
    BAD(rows_ok(M, 1) && D > 0 && D <= 4096 && ld_ok(D, ldx) && ld_ok(D, ldo) && (!has_add || ld_ok(D, ldadd)), "shape out of range");
    const std::vector<float> x = in.f32((long long)M * ldx, "x");
    std::vector<float> add;
    if (has_add) add = in.f32((long long)M * ldadd, "add");
    const std::vector<float> g = in.f32(D, "gamma"), b = in.f32(D, "beta");
    n0 = (size_t)(M + 8) * ldo;
    d0 = pool.filled(n0);
    in.guarded([&] {
      launch_rd_layernorm({pool.up(x), ldx, has_add ? pool.up(add) : nullptr, ldadd, pool.up(g), pool.up(b), 1e-6f, d0, ldo, M, D}, s);
    });
  } else if (op == 6) {
    const int B = h[0], T = h[1], H = h[2], dh = h[3], ld = h[4], ldo = h[5];
    BAD(rows_ok(B, T) && H > 0 && H <= 16 && dh > 0 && dh <= 256 && ld_ok(3 * H * dh, ld) && ld_ok(H * dh, ldo), "shape out of range");
    const long long M = (long long)B * T;
    const std::vector<float> qkv = in.f32(M * ld, "qkv");
    n0 = (size_t)(M + 8) * ldo;
    d0 = pool.filled(n0);
    in.guarded([&] { launch_rd_attn({pool.up(qkv), ld, B, T, H, dh, 1.f / std::sqrt((float)dh), d0, ldo}, s); });
  } else if (op == 7) {
    const int M = h[0], D = h[1], ldx = h[2];
    BAD(rows_ok(M, 1) && ld_ok(D, ldx), "shape out of range");
    const std::vector<float> x = in.f32((long long)M * ldx, "x");
    n0 = (size_t)M * ldx;
    d0 = pool.up(x);
    in.guarded([&] { launch_rd_gelu_tanh(d0, ldx, M, D, s); });
  } else {
    BAD(false, "unknown operator");
  }
  in.result(d0, n0);
}

}  // namespace

int main(int argc, char** argv) { return op_runner_main(argc, argv, "redimnet_oprun", 0x44505357u, Layout{8, 0, 1}, run_case); }
