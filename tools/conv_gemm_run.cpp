// Op-level runner for the implicit-GEMM conv kernels (tests/test_gpu_conv_gemm_op.py).
// Launches the dispatchers of libwsp_hip.so (launch_conv_gemm, launch_conv_gemm_x3,
// conv_gemm_x3_block_rows, launch_colsum_mean).  The float64 reference and the error bound live in
// tests/conv_gemm_ref.py.  Weights arrive in torch layout and go through the project's own
// pack::conv_kmajor / pack::split, so the packer is under test as well.  Framing, case and result
// files: tools/op_runner.h.  Magic 'WSPC' (0x43505357).
//
//   op 1  conv_gemm
//   hdr (42 ints and one f32), in this order:
//        variant (3..7; ignored for precision 0), precision (0 = f32 kernel, 1 = bf16x3), flags,
//        lda[3], cseg[4], cin, taps, dil, pad, M, T, N, ldres, ldo, act, amode, role, conv2d,
//        Fi, Ti, Fo, To, stride, kw, sc2d, gcols, gcin, nseg, lnmode, ln_parts,
//        arows[3]  rows of A buffer i (the buffer holds arows[i] * lda[i] floats),
//        aoff[3]   first float of the operand inside each row (a view into a wider buffer),
//        B         utterances (rows of row_bias and of the column means)
//        ln_eps    f32, in the header's last word
//   arrays, only where the flag bit is set, in this order:
//        bit 0..2  a[0..2]      f32 [arows][lda]
//        (always)  w            f32 [N][cin][taps]   torch layout (2-D: [N][cin][kh][kw])
//        bit 3     bias         f32 [N]
//        bit 4     row_bias     f32 [B][N]
//        bit 5     res          f32 [M][ldres]
//        bit 6     scale, shift f32 [N] each
//        bit 7     seg          i32 [nseg + 1]
//        bit 8     iseg         i32 [nseg + 1]
//        bit 9     (no array)   column sums asked for
//        bit 10    ln_in        f32 [M][ln_parts][2]
//        bit 11    ln_cs        f32 [N]
//        bit 12    ln_g, ln_b   f32 [N] each
//   The header is checked against the rows / columns the kernels will read.
//   K = cin * taps; Kp = K rounded up to 64.
//   results, always three:
//        out [(M + 8)][ldo]   guard rows and guard columns must come back untouched,
//        means [B][N]         launch_colsum_mean of the partials (empty without bit 9),
//        ln_out [M][N/128][2] (empty unless lnmode & 1).
//   own words of the result record (7): char tile[24], i32 block_rows, written for refused cases
//   too.  `tile` names the kernel that served the launch: "g256" where wsp::x3::g256_supported takes
//   the operands under variant 7, else the tile launch_conv_gemm_x3 / launch_conv_gemm pick;
//   block_rows is 0 without bit 9.
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "../wespeaker_hubert_amd/csrc/kernels.h"
#include "../wespeaker_hubert_amd/csrc/pack.h"
#include "op_runner.h"

namespace wsp {
namespace x3 {
bool g256_supported(const ConvGemmArgs&);  // exported by libwsp_hip.so (conv_gemm_x3_t6.hip)
}
}  // namespace wsp

using namespace wsp;

namespace {

constexpr uint32_t kOpConvGemm = 1;
enum {
  H_VARIANT, H_PRECISION, H_FLAGS, H_LDA0, H_LDA1, H_LDA2, H_CSEG0, H_CSEG1, H_CSEG2, H_CSEG3, H_CIN, H_TAPS,
  H_DIL, H_PAD, H_M, H_T, H_N, H_LDRES, H_LDO, H_ACT, H_AMODE, H_ROLE, H_CONV2D, H_FI, H_TI, H_FO, H_TO, H_STRIDE,
  H_KW, H_SC2D, H_GCOLS, H_GCIN, H_NSEG, H_LNMODE, H_LNPARTS, H_AROWS0, H_AROWS1, H_AROWS2, H_AOFF0, H_AOFF1,
  H_AOFF2, H_B, kNH
};
enum {
  F_A0 = 1, F_A1 = 2, F_A2 = 4, F_BIAS = 8, F_ROWBIAS = 16, F_RES = 32, F_SCALE = 64, F_SEG = 128, F_ISEG = 256,
  F_COLSUM = 512, F_LNIN = 1024, F_LNCS = 2048, F_LNGB = 4096
};

// The tile launch_conv_gemm_x3 picks for operands family 7 does not take (conv_gemm_x3.hip).
const char* x3_tile(const ConvGemmArgs& p, int variant) {
  if (variant == 7) variant = 6;
  if (p.N % 64 != 0 || (p.gcols && p.gcols % 64 != 0)) return "128x32";
  if (p.gcols) return variant >= 5 ? "256x64" : "128x64";
  if (p.N % 128 != 0) return "128x64";
  if (variant == 3) return "128x128";
  if (variant == 4) return "256x128";
  if (p.N % 256 == 0) return variant == 6 ? "256x256mf16" : "256x256";
  return "256x128";
}

void run_conv_gemm(Case& in) {
  BAD(in.op == kOpConvGemm, "unknown operator");
  const int* h = in.h;
  Pool& pool = in.pool;
  hipStream_t s = in.stream;
  float ln_eps;
  std::memcpy(&ln_eps, &h[kNH], 4);
  const int flags = h[H_FLAGS], M = h[H_M], T = h[H_T], N = h[H_N], cin = h[H_CIN], taps = h[H_TAPS];
  const int ldo = h[H_LDO], B = h[H_B], nseg = h[H_NSEG];
  BAD(M > 0 && M < (1 << 20) && T > 0 && N > 0 && N <= 4096 && N % 32 == 0, "M / T / N out of range");
  BAD(cin > 0 && cin <= 4096 && cin % 4 == 0 && taps > 0 && taps <= 64, "cin / taps out of range");
  BAD(ldo >= N && ldo <= 8192, "ldo < N");
  BAD(B > 0 && B <= M, "bad utterance count");
  BAD(h[H_PRECISION] == 0 || h[H_PRECISION] == 1, "precision must be 0 or 1");
  BAD(h[H_DIL] >= 0 && h[H_DIL] <= 64 && h[H_PAD] >= 0 && h[H_PAD] <= 4096, "dil / pad out of range");
  BAD(flags & F_A0, "a[0] is required");
  const int K = cin * taps, Kp = (K + 63) / 64 * 64;

  // input rows each operand must hold, from the geometry (not from what the test claims)
  long long need[3] = {0, 0, 0};
  std::vector<int> seg, iseg;
  const bool c2d = h[H_CONV2D] != 0, sc2d = h[H_SC2D] != 0;
  if (c2d || sc2d) {
    BAD(h[H_FO] > 0 && h[H_TO] > 0 && h[H_FI] > 0 && h[H_TI] > 0 && h[H_STRIDE] >= 1, "bad 2-D geometry");
    BAD(M % (h[H_FO] * h[H_TO]) == 0 && M / (h[H_FO] * h[H_TO]) == B, "M != B * Fo * To");
    BAD((h[H_FO] - 1) * h[H_STRIDE] < h[H_FI] + h[H_PAD] && (h[H_TO] - 1) * h[H_STRIDE] < h[H_TI] + h[H_PAD],
        "2-D output larger than its input");
    const long long rows2d = (long long)B * h[H_FI] * h[H_TI];
    need[0] = sc2d ? M : rows2d;
    need[1] = sc2d ? rows2d : 0;
    BAD(!(flags & (F_SEG | F_ISEG)), "2-D cases are uniform");
  }
  std::vector<float> a[3];
  for (int i = 0; i < 3; ++i) {
    BAD(h[H_LDA0 + i] >= 0 && h[H_LDA0 + i] <= 8192 && h[H_AROWS0 + i] >= 0 && h[H_AROWS0 + i] < (1 << 21),
        "lda / arows out of range");
    if (flags & (F_A0 << i)) a[i] = in.f32((long long)h[H_AROWS0 + i] * h[H_LDA0 + i], "a");
  }
  const std::vector<float> w = in.f32((long long)N * cin * taps, "w");
  std::vector<float> bias, row_bias, res, scale, shift, ln_in, ln_cs, ln_g, ln_b;
  if (flags & F_BIAS) bias = in.f32(N, "bias");
  if (flags & F_ROWBIAS) row_bias = in.f32((long long)B * N, "row_bias");
  if (flags & F_RES) {
    BAD(h[H_LDRES] >= N && h[H_LDRES] <= 8192, "ldres < N");
    res = in.f32((long long)M * h[H_LDRES], "res");
  }
  if (flags & F_SCALE) {
    scale = in.f32(N, "scale");
    shift = in.f32(N, "shift");
  }
  auto check_seg = [&](const std::vector<int>& v, const char* what) {
    BAD(v[0] == 0, std::string(what) + "[0] != 0");
    for (int i = 0; i < nseg; ++i) BAD(v[i + 1] > v[i], std::string(what) + " must increase");
  };
  if (flags & F_SEG) {
    BAD(nseg >= 1 && nseg == B, "nseg != B");
    seg = in.i32(nseg + 1, "seg");
    check_seg(seg, "seg");
    BAD(seg[nseg] == M, "seg[nseg] != M");
  }
  if (flags & F_ISEG) {
    BAD(flags & F_SEG, "iseg without seg");
    iseg = in.i32(nseg + 1, "iseg");
    check_seg(iseg, "iseg");
  }
  if (flags & F_LNIN) {
    BAD(h[H_LNPARTS] >= 1 && h[H_LNPARTS] <= 8, "ln_parts out of range");
    ln_in = in.f32((long long)M * h[H_LNPARTS] * 2, "ln_in");
  }
  if (flags & F_LNCS) ln_cs = in.f32(N, "ln_cs");
  if (flags & F_LNGB) {
    ln_g = in.f32(N, "ln_g");
    ln_b = in.f32(N, "ln_b");
  }
  if (!c2d && !sc2d) {
    const int Ti = h[H_TI] > 0 ? h[H_TI] : T;
    if (flags & F_SEG) {
      need[0] = (flags & F_ISEG) ? iseg[nseg] : M;
    } else {
      BAD(M % T == 0 && M / T == B, "M != B * T");
      need[0] = (long long)B * Ti;
    }
    need[1] = need[2] = need[0];
  }
  // columns each operand must hold inside a row
  const bool aadd = h[H_AMODE] == kAAdd;
  BAD(h[H_AMODE] == kACat || aadd, "amode must be 0 or 1");
  BAD(h[H_CSEG0] == 0 && h[H_CSEG1] >= 0 && h[H_CSEG1] <= h[H_CSEG2] && h[H_CSEG2] <= h[H_CSEG3] && h[H_CSEG3] == cin,
      "bad channel segments");
  BAD(h[H_GCOLS] >= 0 && h[H_GCIN] >= 0 && (!h[H_GCOLS] || N % h[H_GCOLS] == 0), "bad grouped columns");
  for (int i = 0; i < 3; ++i) {
    int width = aadd ? (i < 2 ? cin : 0) : h[H_CSEG1 + i] - h[H_CSEG0 + i];
    if (h[H_GCOLS] && i == 0) width = (N / h[H_GCOLS] - 1) * h[H_GCIN] + cin;
    if (width == 0) continue;
    BAD(flags & (F_A0 << i), "an operand the case reads is missing");
    BAD(h[H_AOFF0 + i] >= 0 && h[H_AOFF0 + i] % 4 == 0 && h[H_AOFF0 + i] + width <= h[H_LDA0 + i],
        "operand columns leave the buffer row");
    BAD(h[H_AROWS0 + i] >= need[i], "operand buffer has fewer rows than the case reads");
  }

  // ---- pack and upload
  const std::vector<float> packed = pack::conv_kmajor(w, N, cin, taps, Kp);
  std::vector<uint16_t> whi, wlo;
  pack::split(packed, whi, wlo);
  ConvGemmArgs p{};
  for (int i = 0; i < 3; ++i) {
    const bool have = (flags & (F_A0 << i)) != 0;
    const float* d = have ? pool.up(a[i]) + h[H_AOFF0 + i] : p.a[0];
    p.a[i] = d;
    p.lda[i] = have ? h[H_LDA0 + i] : p.lda[0];
  }
  for (int i = 0; i < 4; ++i) p.cseg[i] = h[H_CSEG0 + i];
  p.cin = cin, p.taps = taps, p.dil = h[H_DIL], p.pad = h[H_PAD];
  p.M = M, p.T = T, p.N = N, p.K = K, p.Kp = Kp;
  p.w = pool.up(packed);
  const uint16_t* dhi = pool.up(whi);
  const uint16_t* dlo = pool.up(wlo);
  if (flags & F_BIAS) p.bias = pool.up(bias);
  if (flags & F_ROWBIAS) p.row_bias = pool.up(row_bias);
  if (flags & F_RES) p.res = pool.up(res), p.ldres = h[H_LDRES];
  if (flags & F_SCALE) p.scale = pool.up(scale), p.shift = pool.up(shift);
  if (flags & F_SEG) p.seg = pool.up(seg), p.nseg = nseg;
  if (flags & F_ISEG) p.iseg = pool.up(iseg);
  p.ldo = ldo, p.act = h[H_ACT], p.amode = h[H_AMODE], p.role = h[H_ROLE];
  p.conv2d = h[H_CONV2D], p.Fi = h[H_FI], p.Ti = h[H_TI], p.Fo = h[H_FO], p.To = h[H_TO];
  p.stride = h[H_STRIDE], p.kw = h[H_KW], p.sc2d = h[H_SC2D], p.gcols = h[H_GCOLS], p.gcin = h[H_GCIN];
  p.lnmode = h[H_LNMODE], p.ln_parts = h[H_LNPARTS], p.ln_eps = ln_eps;
  if (flags & F_LNIN) p.ln_in = pool.up(ln_in);
  if (flags & F_LNCS) p.ln_cs = pool.up(ln_cs);
  if (flags & F_LNGB) p.ln_g = pool.up(ln_g), p.ln_b = pool.up(ln_b);

  const size_t nout = (size_t)(M + 8) * ldo;
  p.out = pool.filled(nout);
  const int variant = h[H_VARIANT], precision = h[H_PRECISION];
  int bm = 0;
  double* dpart = nullptr;
  size_t nln = 0;
  if (flags & F_COLSUM) {
    bm = precision ? conv_gemm_x3_block_rows(p, variant) : 128;
    BAD(bm == 128 || bm == 256, "unexpected block rows");
    std::vector<uint64_t> nanfill((size_t)((M + bm - 1) / bm) * 2 * N, 0x7FF8A5A5A5A5A5A5ull);
    dpart = reinterpret_cast<double*>(pool.up(nanfill));
    p.colsum = dpart;
  }
  if (p.lnmode & 1) {
    BAD(N % 128 == 0, "ln_out needs N % 128 == 0");
    nln = (size_t)M * (N / 128) * 2;
    p.ln_out = pool.filled(nln);
  }

  // ---- launch through the library's dispatchers
  const char* tile = "";
  float* dmeans = nullptr;
  in.guarded([&] {
    if (precision == 0) {
      tile = (conv_gemm_tile_for(N) == 0 && !p.gcols) ? "f32_128x128" : "f32_128x64";
      launch_conv_gemm(p, s);
    } else {
      tile = (variant == 7 && x3::g256_supported(normalized(p))) ? "g256" : x3_tile(p, variant);
      launch_conv_gemm_x3(p, dhi, dlo, variant, s);
    }
    if (flags & F_COLSUM) {
      dmeans = pool.filled((size_t)B * N);
      launch_colsum_mean(dpart, bm, T, B, N, dmeans, N, s);
    }
  });
  std::snprintf(reinterpret_cast<char*>(in.own), 24, "%s", tile);
  in.own[6] = (uint32_t)bm;
  in.note = "precision " + std::to_string(precision) + " variant " + std::to_string(variant) + " M " + std::to_string(M) +
            " N " + std::to_string(N) + " K " + std::to_string(K) + " tile " + tile;  // the stdout line
  in.result(p.out, nout);
  in.result(dmeans, dmeans ? (size_t)B * N : 0);
  in.result(p.ln_out, nln);
}

}  // namespace

static_assert(kNH + 1 == 43, "the header: kNH ints and ln_eps");
int main(int argc, char** argv) { return op_runner_main(argc, argv, "conv_gemm_run", 0x43505357u, Layout{43, 7, 3}, run_conv_gemm); }
