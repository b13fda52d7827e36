// Internal: what the families on eres2net.hip's transposed-MFMA convs share on the host (ERes2Net,
// Res2Net): a conv with its eval BatchNorm folded in (Impl::fold_bn: the scale in float64), k-major,
// as pack::frag16 fragments + bias.
#pragma once

#include "model_impl.h"

namespace wsp {

struct Pw {  // BN-folded conv as pack::frag16 fragments + bias
  void* w = nullptr;
  float* b = nullptr;
  int N = 0, K = 0;
};

// conv [N][cin][taps] -> BN folded, k = tap * cin + c, as eres2net.hip fragments; acc_order: the k
// order of pack::frag16(acc_order), for a product whose other operand is accumulator tiles
inline Pw fold_pw(Model::Impl& m, const std::string& wname, const std::string& bn, int N, int cin, int taps,
                  bool acc_order = false) {
  const Model::Impl::Folded f = m.fold_bn(wname, bn);
  Pw pw;
  pw.N = N;
  pw.K = cin * taps;
  const std::vector<float> wk = pack::conv_kmajor(f.w, N, cin, taps, pw.K);
  pw.w = m.dev.upload_u16(pack::frag16(wk.data(), N, pw.K, pw.K, acc_order));
  pw.b = m.dev.upload(f.b);
  return pw;
}

}  // namespace wsp
