// Op-level runner for the ResNet / SimAM-ResNet kernels (tests/test_gpu_resnet_op.py).
// Launches launch_conv3x3_img, launch_bottleneck_tail, launch_resnet_stem, launch_simam and
// launch_nhwc_to_tfc of libwsp_hip.so and, as conv3x3's twin, launch_conv_gemm_x3 in conv2d mode.  Weights
// arrive in torch layout and are packed with the library's own packers as resnet_model.cpp packs them:
// conv2 and the fused next conv1 with pack::frag(pack::conv_kmajor(...)), conv3 with pack::kAcc, the
// [conv3 | shortcut] image of the in-tail shortcut with pack::kAcc and kacc = planes, the implicit GEMM's
// operands with pack::conv_kmajor + pack::split.  Framing, case and result files: tools/op_runner.h.
// Magic 'WSPN' (0x4E505357).  Arrays are f32.  An array the header switches off arrives empty.
//
//   op 1  conv3x3      hdr = C, B, F, T, variant, relu, has_res, has_scale, twin, gemm_variant
//         arrays x [B][F][T][C], W [C][C][3][3] (torch layout), bias [C], res [B][F][T][C] (or empty),
//         scale [C], shift [C] (or both empty)
//         results out [(M + 8)][C] of launch_conv3x3_img (M = B F T; the launch gets row 4), then the same
//         buffer of launch_conv_gemm_x3 (conv2d, 3x3, pad 1, stride 1) on the same operands (empty when
//         twin = 0)
//   op 2  bottleneck_tail   hdr = C, B, F, T, fuse1, c1n, xsc, alias, with_res, both
//         arrays y1 [B][F][T][C], res [B][F][T][4C] (empty when with_res = 0), W2 [C][C][3][3], b2 [C],
//         W3 [4C][C] (xsc: [4C][2C] = [conv3 | shortcut]), b3 [4C], W1 [c1n][4C], b1 [c1n] (both empty when
//         fuse1 = 0), xs [B][F][T][C] (empty when xsc = 0)
//         results out [(M + 8)][4C], y1n [(M + 8)][c1n] (empty when fuse1 = 0), and, both = 1, out
//         [(M + 8)][4C] of a second launch without the next conv1 (else empty): the launch gets row 4 of each
//         alias = 1: res is the out pointer itself (the launcher must refuse)
//   op 3  resnet_stem  hdr = B, T, F, C0
//         arrays feats [B][T][F], w [C0][9], bias [C0];  result out [(B F T + 8)][C0]: the launch gets row 4
//   op 4  simam        hdr = B, rows, C
//         arrays z [B][rows][C], res [B][rows][C]
//         results out [(B rows + 8)][C] (the launch gets row 4), coef [B][2][C] (the kernel's own mean and
//         1 / (4 (var + 1e-4)), held to the float64 statistics as well)
//   op 5  nhwc_to_tfc  hdr = B, F, T, C
//         arrays in [B][F][T][C];  result out [(B F T + 8)][C]: the launch gets row 4
// Guard rows must come back untouched.
#include <algorithm>
#include <vector>

#include "../wespeaker_hubert_amd/csrc/conv3x3_img.h"
#include "../wespeaker_hubert_amd/csrc/kernels.h"
#include "../wespeaker_hubert_amd/csrc/pack.h"
#include "op_runner.h"

using namespace wsp;

namespace {

constexpr long long kMaxPos = 1 << 14;  // positions (B F T) of a case
constexpr int kGuard = 4;               // guard rows on either side of an output

void image_shape(const int* h, const char* what) {
  const int C = h[0], B = h[1], F = h[2], T = h[3];
  BAD(C >= 32 && C <= 128 && C % 32 == 0 && B >= 1 && B <= 64 && F >= 1 && F <= 256 && T >= 1 && T <= 4096 &&
          (long long)B * F * T <= kMaxPos,
      std::string(what) + ": shape");
}

bool flag(int v) { return v == 0 || v == 1; }

void run_conv3x3(Case& c) {
  const int* h = c.h;
  const int C = h[0], B = h[1], F = h[2], T = h[3], variant = h[4], relu = h[5], has_res = h[6], has_scale = h[7],
            twin = h[8], gv = h[9];
  image_shape(h, "conv3x3");
  BAD(flag(relu) && flag(has_res) && flag(has_scale) && flag(twin) && variant >= 0 && variant <= 3 && gv >= 3 && gv <= 7,
      "conv3x3: flags");
  const long long M = (long long)B * F * T;
  const auto x = c.f32(M * C, "x"), W = c.f32((long long)C * C * 9, "W"), bias = c.f32(C, "bias");
  const auto res = c.f32(has_res ? M * C : 0, "res");
  const auto scale = c.f32(has_scale ? C : 0, "scale"), shift = c.f32(has_scale ? C : 0, "shift");
  Pool& pool = c.pool;
  const size_t n = (size_t)(M + 2 * kGuard) * C;
  float* out = pool.filled(n);
  float* out2 = twin ? pool.filled(n) : nullptr;
  c.result(out, n);
  c.result(out2, twin ? n : 0);
  c.guarded([&] {
    const int K = 9 * C, Kp = (K + 63) / 64 * 64;
    const float* dx = pool.up(x);
    const float* db = pool.up(bias);
    const float* dres = has_res ? pool.up(res) : nullptr;
    const float* dsc = has_scale ? pool.up(scale) : nullptr;
    const float* dsh = has_scale ? pool.up(shift) : nullptr;
    Conv3x3Args a{dx, out + kGuard * (size_t)C, B, F, T, pool.up(pack::frag(pack::conv_kmajor(W, C, C, 9, K), C, K)),
                  db, dsc, dsh, dres, relu, variant};
    launch_conv3x3_img(a, C, c.stream);
    if (!twin) return;
    const std::vector<float> packed = pack::conv_kmajor(W, C, C, 9, Kp);
    std::vector<uint16_t> whi, wlo;
    pack::split(packed, whi, wlo);
    ConvGemmArgs g{};
    g.a[0] = g.a[1] = g.a[2] = dx;
    g.lda[0] = g.lda[1] = g.lda[2] = C;
    g.cseg[1] = g.cseg[2] = g.cseg[3] = C;
    g.cin = C, g.taps = 9, g.dil = 1, g.pad = 1, g.M = (int)M, g.T = (int)M, g.N = C, g.K = K, g.Kp = Kp;
    g.w = pool.up(packed);
    g.bias = db, g.scale = dsc, g.shift = dsh, g.res = dres, g.ldres = has_res ? C : 0;
    g.out = out2 + kGuard * (size_t)C, g.ldo = C, g.act = relu ? kActRelu : kActNone, g.amode = kACat;
    g.conv2d = 1, g.Fi = g.Fo = F, g.Ti = g.To = T, g.stride = 1, g.kw = 3;
    launch_conv_gemm_x3(g, pool.up(whi), pool.up(wlo), gv, c.stream);
  });
}

void run_tail(Case& c) {
  const int* h = c.h;
  const int C = h[0], B = h[1], F = h[2], T = h[3], fuse1 = h[4], c1n = h[5], xsc = h[6], alias = h[7], with_res = h[8],
            both = h[9];
  image_shape(h, "tail");
  BAD(flag(fuse1) && flag(xsc) && flag(alias) && flag(with_res) && flag(both), "tail: flags");
  BAD(fuse1 ? (c1n == C || c1n == 2 * C) : c1n == 0, "tail: c1n");
  BAD((!alias || with_res) && (!both || (fuse1 && with_res && !xsc && !alias)), "tail: alias / both");
  const long long M = (long long)B * F * T;
  const int C4 = 4 * C, K3 = xsc ? 2 * C : C;
  const auto y1 = c.f32(M * C, "y1"), res = c.f32(with_res ? M * C4 : 0, "res");
  const auto W2 = c.f32((long long)C * C * 9, "W2"), b2 = c.f32(C, "b2");
  const auto W3 = c.f32((long long)C4 * K3, "W3"), b3 = c.f32(C4, "b3");
  const auto W1 = c.f32(fuse1 ? (long long)c1n * C4 : 0, "W1"), b1 = c.f32(fuse1 ? c1n : 0, "b1");
  const auto xs = c.f32(xsc ? M * C : 0, "xs");
  Pool& pool = c.pool;
  const size_t n = (size_t)(M + 2 * kGuard) * C4, n1 = fuse1 ? (size_t)(M + 2 * kGuard) * c1n : 0;
  float* out = pool.filled(n);
  float* y1n = fuse1 ? pool.filled(n1) : nullptr;
  float* out_plain = both ? pool.filled(n) : nullptr;
  c.result(out, n);
  c.result(y1n, n1);
  c.result(out_plain, both ? n : 0);
  c.guarded([&] {
    BottleneckTailArgs a{};
    a.y1 = pool.up(y1);
    a.out = out + kGuard * (size_t)C4;
    a.res = alias ? a.out : with_res ? pool.up(res) : nullptr;
    a.B = B, a.F = F, a.T = T;
    a.w2 = pool.up(pack::frag(pack::conv_kmajor(W2, C, C, 9, 9 * C), C, 9 * C));
    a.b2 = pool.up(b2);
    a.w3 = pool.up(xsc ? pack::frag(W3, C4, K3, pack::kAcc, C) : pack::frag(W3, C4, C, pack::kAcc));
    a.b3 = pool.up(b3);
    if (fuse1) {
      a.w1n = pool.up(pack::frag(pack::conv_kmajor(W1, c1n, C4, 1, C4), c1n, C4));
      a.b1n = pool.up(b1);
      a.y1n = y1n + kGuard * (size_t)c1n;
      a.c1n = c1n;
    }
    if (xsc) a.xsc = pool.up(xs);
    launch_bottleneck_tail(a, C, c.stream);
    if (!both) return;
    BottleneckTailArgs p = a;
    p.out = out_plain + kGuard * (size_t)C4;
    p.w1n = nullptr, p.b1n = nullptr, p.y1n = nullptr, p.c1n = 0;
    launch_bottleneck_tail(p, C, c.stream);
  });
}

void run_stem(Case& c) {
  const int* h = c.h;
  const int B = h[0], T = h[1], F = h[2], C0 = h[3];
  BAD(B >= 1 && B <= 64 && T >= 1 && T <= 4096 && F >= 1 && F <= 256 && (long long)B * F * T <= kMaxPos && C0 >= 4 &&
          C0 <= 64 && C0 % 4 == 0,
      "stem: shape");
  const long long M = (long long)B * F * T;
  const auto feats = c.f32(M, "feats"), w = c.f32(C0 * 9, "w"), bias = c.f32(C0, "bias");
  Pool& pool = c.pool;
  const size_t n = (size_t)(M + 2 * kGuard) * C0;
  float* out = pool.filled(n);
  c.result(out, n);
  c.guarded([&] {
    launch_resnet_stem(pool.up(feats), B, T, F, C0, pool.up(w), pool.up(bias), out + kGuard * (size_t)C0, c.stream);
  });
}

void run_simam(Case& c) {
  const int* h = c.h;
  const int B = h[0], rows = h[1], C = h[2];
  BAD(B >= 1 && B <= 64 && rows >= 1 && rows <= 8192 && C >= 4 && C <= 1024 && C % 4 == 0 &&
          (long long)B * rows * C <= (1 << 20),
      "simam: shape");
  const long long n = (long long)B * rows * C;
  const auto z = c.f32(n, "z"), res = c.f32(n, "res");
  Pool& pool = c.pool;
  const size_t no = (size_t)n + 2 * kGuard * (size_t)C, nc = (size_t)B * 2 * C;
  float* out = pool.filled(no);
  float* coef = pool.filled(nc);
  c.result(out, no);
  c.result(coef, nc);
  c.guarded([&] {
    double* part = pool.up(std::vector<double>((size_t)B * simam_chunks(B, rows) * 2 * C, 0.0));
    launch_simam(pool.up(z), pool.up(res), out + kGuard * (size_t)C, B, rows, C, part, coef, c.stream);
  });
}

void run_tfc(Case& c) {
  const int* h = c.h;
  const int B = h[0], F = h[1], T = h[2], C = h[3];
  BAD(B >= 1 && B <= 64 && F >= 1 && F <= 256 && T >= 1 && T <= 4096 && C >= 4 && C <= 1024 && C % 4 == 0 &&
          (long long)B * F * T * C <= (1 << 20),
      "nhwc_to_tfc: shape");
  const long long n = (long long)B * F * T * C;
  const auto in = c.f32(n, "in");
  Pool& pool = c.pool;
  const size_t no = (size_t)n + 2 * kGuard * (size_t)C;
  float* out = pool.filled(no);
  c.result(out, no);
  c.guarded([&] { launch_nhwc_to_tfc(pool.up(in), out + kGuard * (size_t)C, B, F, T, C, c.stream); });
}

void run_case(Case& c) {
  switch (c.op) {
    case 1: run_conv3x3(c); break;
    case 2: run_tail(c); break;
    case 3: run_stem(c); break;
    case 4: run_simam(c); break;
    case 5: run_tfc(c); break;
    default: BAD(false, "unknown operator");
  }
}

}  // namespace

int main(int argc, char** argv) { return op_runner_main(argc, argv, "resnet_run", 0x4e505357u, Layout{16, 0, 0}, run_case); }
