// rj_model.hpp — the record-row writer and the model's host expressions: the
// metric H(q), the kinetic energy, RandomState.choice and the Beta density.
// Plain C++ and np_legacy.hpp; a section of rhmc_rj.cpp's translation unit.
#pragma once

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <vector>

#include <emmintrin.h>

#include "np_legacy.hpp"
#include "rhmc_rj.h"

namespace {

constexpr double kPi = 3.141592653589793;  // np.pi

// ------------------------------------------------------------ record rows
// One [3 N_max] row of a record or of the final states: src[0, d) then zeros
// to `zero_to` (W, or less where the caller's row is known to be zero past it:
// rhmc_rj_config::records_zero_padded).  A full row goes out with
// non-temporal stores: the q_chain / p_chain records are 2 x 3 N_max doubles
// per chain and iteration (24 MB per iteration at 4,096 chains and N_max 120,
// most of it the zero padding), written once and not read back by the run;
// plain stores first pull every destination line into the cache, which
// halved the host's record bandwidth (tools/rec_write_bench.cpp).  The
// caller issues _mm_sfence() before the rows are handed on.
void put_row(double* dst, const double* src, int64_t d, int64_t zero_to, int64_t W) {
  if (zero_to < W) {
    std::fill(std::copy(src, src + d, dst), dst + zero_to, 0.);
    return;
  }
  int64_t i = 0;
  if (reinterpret_cast<uintptr_t>(dst) & 15) {  // to a 16-byte boundary
    dst[0] = d > 0 ? src[0] : 0.;
    i = 1;
  }
  for (; i + 2 <= d; i += 2) _mm_stream_pd(dst + i, _mm_loadu_pd(src + i));
  if (i < d) {  // one live value left
    if (i + 2 <= W) {
      _mm_stream_pd(dst + i, _mm_set_pd(0., src[i]));
      i += 2;
    } else {
      dst[i] = src[i];
      ++i;
    }
  }
  const __m128d z = _mm_setzero_pd();
  for (; i + 2 <= W; i += 2) _mm_stream_pd(dst + i, z);
  if (i < W) dst[i] = 0.;
}

// The zero fill's end for record row r: with records_zero_padded the row
// holds zeros past 3 n_stars[r] (the previous run's count), so the fill stops
// at the larger of that and the new width d; else the whole row
int64_t zero_end(const rhmc_rj_config* cfg, const rhmc_rj_record* rec, int64_t r, int64_t d,
                 int64_t W) {
  if (!(cfg->records_zero_padded & RHMC_RJ_ZP_RECORDS)) return W;
  const int32_t old = rec->n_stars[r];
  if (old < 1 || old > cfg->N_max) return W;
  return std::max(d, 3 * (int64_t)old);
}

// ------------------------------------------------------------ model helpers
// H(q) of one star (sampler.py _H_vec, sampler_RHMC.py:260-292): Hd = (H_ff,
// H_xx, H_xx).
struct Metric {
  double g_ff2, g_ff, g_xx, g0, g1, g2, B, f_low;
  void star(double f, double* Hd) const {
    const double Hf = 1. / (f / g_ff2 + (B / g0) / g_ff);
    const double fl = f < f_low ? f_low : f;
    const double s = 1. / (g1 * fl) + B / (g2 * (fl * fl));
    const double Hx = g_xx * (1. / s);
    Hd[0] = Hf;
    Hd[1] = Hx;
    Hd[2] = Hx;
  }
  void all(const double* q, int64_t d, double* Hd) const {
    for (int64_t i = 0; i < d; i += 3) star(q[i], Hd + i);
  }
};

// T(p, H) = (sum p^2 / H + sum ln|H|) / 2 with NumPy's pairwise sums (:353-363)
double kinetic(const double* p, const double* H, int64_t d, std::vector<double>& tmp) {
  tmp.resize((size_t)d);
  for (int64_t i = 0; i < d; ++i) tmp[i] = (p[i] * p[i]) / H[i];
  const double s1 = rhmc_np::pairwise_sum(tmp.data(), d);
  for (int64_t i = 0; i < d; ++i)  // a star's two position entries share H: one log
    tmp[i] = (i % 3 == 2 && H[i] == H[i - 1]) ? tmp[i - 1] : std::log(std::fabs(H[i]));
  const double s2 = rhmc_np::pairwise_sum(tmp.data(), d);
  return (s1 + s2) / 2.;
}

// RandomState.choice(k, p=w) for one value: cdf = cumsum(w) / cdf[-1], one
// uniform, searchsorted(side='right')
int64_t choice(rhmc_np::Legacy& r, const double* w, int64_t k, std::vector<double>& cdf) {
  cdf.resize((size_t)k);
  double acc = 0.;
  for (int64_t i = 0; i < k; ++i) cdf[i] = acc = acc + w[i];
  const double last = cdf[k - 1];
  for (int64_t i = 0; i < k; ++i) cdf[i] /= last;
  const double u = r.random_sample();
  return std::upper_bound(cdf.begin(), cdf.end(), u) - cdf.begin();
}

// scipy.stats.beta.logpdf / pdf: xlog1py(b-1, -x) + xlogy(a-1, x) - betaln(a, b);
// the pdf with integer exponents as products (the merge evaluates it on every
// star pair: beta_a = beta_b = 2 by default, 6 x (1 - x))
struct BetaDist {
  double a = 2., b = 2., lb = 0., inv_b = 0.;
  int ia = -1, ib = -1;  // a - 1, b - 1 when small non-negative integers
  void set(double a_, double b_) {
    a = a_;
    b = b_;
    lb = std::lgamma(a) + std::lgamma(b) - std::lgamma(a + b);
    inv_b = std::exp(-lb);
    ia = (a - 1 >= 0 && a - 1 <= 8 && a == std::floor(a)) ? (int)(a - 1) : -1;
    ib = (b - 1 >= 0 && b - 1 <= 8 && b == std::floor(b)) ? (int)(b - 1) : -1;
  }
  double logpdf(double x) const {
    const double t1 = (b - 1.0 == 0.0) ? 0.0 : (b - 1.0) * std::log1p(-x);
    const double t2 = (a - 1.0 == 0.0) ? 0.0 : (a - 1.0) * std::log(x);
    return t1 + t2 - lb;
  }
  double pdf(double x) const {
    if (!(x >= 0.0 && x <= 1.0)) return 0.0;
    if (ia >= 0 && ib >= 0) {
      double v = inv_b;
      for (int k = 0; k < ia; ++k) v *= x;
      const double y = 1.0 - x;
      for (int k = 0; k < ib; ++k) v *= y;
      return v;
    }
    return std::exp(logpdf(x));
  }
};

}  // namespace
