// Op-level runner for the kernels only the HuBERT / WavLM front end uses (tests/test_gpu_ssl_op.py).
// Launches launch_attn, launch_attn_gate, launch_hubert_pos_conv, launch_layernorm and
// launch_hubert_conv0 of libwsp_hip.so, with pos_conv's weights packed by the library's own
// pack::conv_kmajor / pack::split as the model packs them.  Framing, case and result files:
// tools/op_runner.h.  Magic 'WSPS' (0x53505357).  Arrays are f32; the offset arrays seg / wseg /
// oseg / fseg are i32.
//
//   op 1  attention     hdr = B, T (longest utterance), H, dh, ldq, ldo, rows, nseg (0: uniform, else B),
//                       pipe, has_bias
//         arrays qkv [rows][ldq], (seg [B + 1]), (table [H][1560], gate [rows][H])
//         results out [(rows + 8)][ldo]
//   op 2  gate          hdr = rows, H, ldx
//         arrays x [rows][ldx], w [130 + H] = wa (64) | wb (64) | ba | bb | grep_a (H)
//         results gate [(rows + 8)][H]
//   op 3  pos_conv      hdr = B, maxT, M, ldx, ldo, gout
//         arrays x [M][ldx], seg [B + 1], w [16 gout][48][128] (torch layout, the padded grouped
//         weight), bias [16 gout];  results out [(M + 8)][ldo]
//   op 4  LayerNorm     hdr = M, D, ldx, ldo, has_add, ldadd, gin, gout, has_feat, feat_init, T, Tout,
//                       nseg, frows (feature rows)
//         arrays x [M][ldx], (add [M][ldadd]), gamma [D], beta [D], params [2] = eps, feat_w,
//         (seg [nseg + 1], fseg [nseg + 1]), (feat [frows][D]: the prior contents, feat_init = 0)
//         results out [(M + 8)][ldo], (feat [(frows + 8)][D])
//   op 5  conv0         hdr = B, N, ldw, T0 (longest utterance's frames), nseg (0: uniform, else B),
//                       wrows (samples in all), orows (frames in all)
//         arrays wav [wrows], w [512][10], gamma [512], beta [512], (wseg [B + 1], oseg [B + 1])
//         results out [(orows + 8)][512]
// Every offset array is checked against the rows it indexes.  Guard rows and guard columns must come
// back untouched.
#include <algorithm>
#include <vector>

#include "../wespeaker_hubert_amd/csrc/attn.h"
#include "../wespeaker_hubert_amd/csrc/kernels.h"
#include "../wespeaker_hubert_amd/csrc/pack.h"
#include "op_runner.h"

using namespace wsp;

namespace {

constexpr long long kMaxRows = 1 << 20;

// offsets of B utterances over `rows` rows: 0 = s[0] < s[1] < ... < s[B] = rows, each at most `longest`
std::vector<int> offsets(Case& in, int B, long long rows, long long longest, const char* what) {
  const std::vector<int> s = in.i32((long long)B + 1, what);
  BAD(s[0] == 0 && s[B] == rows, std::string(what) + ": offsets do not span the rows");
  for (int b = 0; b < B; ++b)
    BAD(s[b + 1] > s[b] && s[b + 1] - s[b] <= longest, std::string(what) + ": utterance length out of range");
  return s;
}

void run_case(Case& in) {
  const uint32_t op = in.op;
  Pool& pool = in.pool;
  hipStream_t s = in.stream;
  float* d[2] = {nullptr, nullptr};
  size_t n[2] = {0, 0};
  if (op == 1) {
    const int* h = in.h;
    const int B = h[0], T = h[1], H = h[2], dh = h[3], ldq = h[4], ldo = h[5], rows = h[6], nseg = h[7], pipe = h[8],
              has_bias = h[9];
    BAD(B > 0 && B <= 4096 && T > 0 && T <= 4096 && H > 0 && H <= 16 && rows > 0 && rows < kMaxRows, "shape out of range");
    BAD(dh > 0 && dh <= 64 && ldq >= 3 * H * 64 && ldq <= 8192 && ldo > 0 && ldo <= 8192, "bad strides");
    BAD((nseg == 0 && rows == B * T) || nseg == B, "rows / nseg do not match the batch");
    BAD((pipe == 0 || pipe == 1) && (has_bias == 0 || has_bias == 1), "bad pipe / bias flag");
    const std::vector<float> qkv = in.f32((long long)rows * ldq, "qkv");
    std::vector<int> seg;
    if (nseg) seg = offsets(in, B, rows, T, "seg");
    std::vector<float> table, gate;
    if (has_bias) {
      table = in.f32((long long)H * kAttnRelStride, "table");
      gate = in.f32((long long)rows * H, "gate");
    }
    n[0] = (size_t)(rows + 8) * std::max(ldo, H * 64);  // a row stride the launcher must refuse stays in bounds
    d[0] = pool.filled(n[0]);
    in.guarded([&] {
      AttnBias ab;
      if (has_bias) ab.table = pool.up(table), ab.gate = pool.up(gate);
      launch_attn(pool.up(qkv), ldq, d[0], ldo, B, T, H, dh, s, nseg ? pool.up(seg) : nullptr, pipe,
                  has_bias ? &ab : nullptr);
    });
  } else if (op == 2) {
    const int* h = in.h;
    const int rows = h[0], H = h[1], ldx = h[2];
    BAD(rows > 0 && rows < kMaxRows && H > 0 && H <= 16 && ldx >= H * 64 && ldx <= 8192, "shape out of range");
    const std::vector<float> x = in.f32((long long)rows * ldx, "x"), w = in.f32(130 + H, "w");
    n[0] = (size_t)(rows + 8) * H;
    d[0] = pool.filled(n[0]);
    in.guarded([&] { launch_attn_gate(pool.up(x), ldx, rows, H, pool.up(w), d[0], s); });
  } else if (op == 3) {
    const int* h = in.h;
    const int B = h[0], maxT = h[1], M = h[2], ldx = h[3], ldo = h[4], gout = h[5];
    constexpr int kG = 16, kCin = 48, kTaps = 128, kK = kCin * kTaps;
    BAD(B > 0 && B <= 4096 && maxT > 0 && M > 0 && M < kMaxRows, "shape out of range");
    BAD(ldx >= kG * kCin && ldx <= 8192 && gout >= kCin && gout <= 128 && ldo >= kG * gout && ldo <= 8192, "bad strides");
    const std::vector<float> x = in.f32((long long)M * ldx, "x");
    const std::vector<int> seg = offsets(in, B, M, maxT, "seg");
    const std::vector<float> w = in.f32((long long)kG * gout * kK, "w"), bias = in.f32(kG * gout, "bias");
    n[0] = (size_t)(M + 8) * ldo;
    d[0] = pool.filled(n[0]);
    in.guarded([&] {
      std::vector<uint16_t> hi, lo;
      pack::split(pack::conv_kmajor(w, kG * gout, kCin, kTaps, kK), hi, lo);
      launch_hubert_pos_conv(pool.up(x), ldx, pool.up(seg), B, maxT, M, pool.up(hi), pool.up(lo), kK, gout,
                             pool.up(bias), d[0], ldo, s);
    });
  } else if (op == 4) {
    const int* h = in.h;
    const int M = h[0], D = h[1], ldx = h[2], ldo = h[3], has_add = h[4], ldadd = h[5], gin = h[6], gout = h[7],
              has_feat = h[8], feat_init = h[9], T = h[10], Tout = h[11], nseg = h[12], frows = h[13];
    BAD(M > 0 && M < kMaxRows && D > 0 && D <= 1024 && ldx > 0 && ldx <= 8192 && ldo > 0 && ldo <= 8192,
        "shape out of range");
    if (has_add) BAD(gin > 0 && gout > 0 && gout <= 1024 && ldadd > 0 && ldadd <= 8192, "bad add remap");
    // strides the launcher must refuse stay in bounds: a row of slack behind x and add, out rows of at least D
    const size_t slack = has_add ? (size_t)((D - 1) / gin) * gout + gin + D : D;
    if (has_feat) {
      BAD(frows > 0 && frows < kMaxRows && nseg >= 0 && nseg <= 4096, "bad feature rows");
      if (!nseg) BAD(T > 0 && Tout > 0 && M % T == 0 && frows == (long long)(M / T) * Tout, "bad featurizer shape");
    } else {
      BAD(nseg == 0 && frows == 0, "segments without a featurizer");
    }
    std::vector<float> x = in.f32((long long)M * ldx, "x");
    std::vector<float> add, prior;
    if (has_add) add = in.f32((long long)M * ldadd, "add");
    x.resize(x.size() + slack, 0.f);
    if (has_add) add.resize(add.size() + slack, 0.f);
    const std::vector<float> gamma = in.f32(D, "gamma"), beta = in.f32(D, "beta"), params = in.f32(2, "params");
    std::vector<int> seg, fseg;
    if (nseg) {
      seg = offsets(in, nseg, M, M, "seg");
      fseg = offsets(in, nseg, frows, frows, "fseg");
    }
    n[0] = (size_t)(M + 8) * std::max(ldo, D);
    d[0] = pool.filled(n[0]);
    if (has_feat) {
      n[1] = (size_t)(frows + 8) * D;
      d[1] = pool.filled(n[1]);
      if (!feat_init) {
        prior = in.f32((long long)frows * D, "feat");
        CK(hipMemcpy(d[1], prior.data(), prior.size() * 4, hipMemcpyHostToDevice));
      }
    }
    in.guarded([&] {
      LayerNormArgs a{};
      a.x = pool.up(x), a.ldx = ldx;
      if (has_add) a.add = pool.up(add), a.ldadd = ldadd, a.gin = gin, a.gout = gout;
      a.gamma = pool.up(gamma), a.beta = pool.up(beta), a.eps = params[0];
      a.out = d[0], a.ldo = ldo, a.M = M, a.D = D;
      if (has_feat) {
        a.feat = d[1], a.feat_w = params[1], a.feat_init = feat_init, a.T = T, a.Tout = Tout;
        if (nseg) a.seg = pool.up(seg), a.fseg = pool.up(fseg), a.nseg = nseg;
      }
      launch_layernorm(a, s);
    });
  } else if (op == 5) {
    const int* h = in.h;
    const int B = h[0], N = h[1], ldw = h[2], T0 = h[3], nseg = h[4], wrows = h[5], orows = h[6];
    BAD(B > 0 && B <= 4096 && T0 > 0 && wrows > 0 && wrows < (1 << 24) && orows > 0 && orows < kMaxRows,
        "shape out of range");
    if (nseg)
      BAD(nseg == B, "nseg does not match the batch");
    else
      BAD(N > 0 && ldw >= N && wrows == (long long)B * ldw && orows == (long long)B * T0, "bad uniform batch");
    const std::vector<float> wav = in.f32(wrows, "wav"), w = in.f32(512 * 10, "w"), gamma = in.f32(512, "gamma"),
                             beta = in.f32(512, "beta");
    std::vector<int> wseg, oseg;
    if (nseg) {
      wseg = offsets(in, B, wrows, wrows, "wseg");
      oseg = offsets(in, B, orows, T0, "oseg");
    }
    n[0] = (size_t)(orows + 8) * 512;
    d[0] = pool.filled(n[0]);
    in.guarded([&] {
      double* stats = pool.up(std::vector<double>(hubert_conv0_stats_doubles(B, T0), 0.0));
      launch_hubert_conv0(pool.up(wav), B, N, ldw, T0, pool.up(w), pool.up(gamma), pool.up(beta), stats, d[0], s,
                          nseg ? pool.up(wseg) : nullptr, nseg ? pool.up(oseg) : nullptr);
    });
  } else {
    BAD(false, "unknown operator");
  }
  in.result(d[0], n[0]);
  if (d[1]) in.result(d[1], n[1]);
}

}  // namespace

int main(int argc, char** argv) { return op_runner_main(argc, argv, "ssl_run", 0x53505357u, Layout{16, 0, 0}, run_case); }
