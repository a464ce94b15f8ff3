// The lag search of convergence_stats (utils.py:141-166) on given variograms:
// host only, no HIP.  rhmc_post_neff exports it; the convergence driver
// applies it per coordinate after every pass.
#pragma once
#include <cmath>
#include <cstdint>
#include <limits>
#include <vector>

namespace rhmc_post {

struct NeffResult {
  double n_eff;
  int32_t decided;   // the rule fired, ran to t = n - 2, or var is degenerate
  int64_t lags;      // variograms read: the reference loop's count when decided
};

// np.sum of a contiguous double array (NumPy's pairwise_sum, 8 accumulators,
// blocks of 128), so that the sum of the rho_t rounds like the reference's.
inline double np_pairwise_sum(const double* a, int64_t n) {
  if (n < 8) {
    double s = 0.;
    for (int64_t i = 0; i < n; ++i) s += a[i];
    return s;
  }
  if (n <= 128) {
    double r[8];
    for (int j = 0; j < 8; ++j) r[j] = a[j];
    int64_t i = 8;
    for (; i < n - (n % 8); i += 8)
      for (int j = 0; j < 8; ++j) r[j] += a[i + j];
    double s = ((r[0] + r[1]) + (r[2] + r[3])) + ((r[4] + r[5]) + (r[6] + r[7]));
    for (; i < n; ++i) s += a[i];
    return s;
  }
  int64_t n2 = n / 2;
  n2 -= n2 % 8;
  return np_pairwise_sum(a, n2) + np_pairwise_sum(a + n2, n - n2);
}

// V[i] = V_{i+1}, i < n_lags; m sequences of length n >= 3.
inline NeffResult neff_rule(int64_t m, int64_t n, double var, const double* V, int64_t n_lags) {
  const double mn = double(m) * double(n);
  if (!(std::isfinite(var) && var > 0.))
    return {std::numeric_limits<double>::quiet_NaN(), 1, 0};
  if (n_lags < 1) return {mn, 0, 0};
  auto rho = [&](int64_t t) { return 1. - V[t - 1] / (2. * var); };
  // the reference evaluates V_1 and V_2 before it looks at rho_1
  if (rho(1) < 5e-2) return {mn, 1, 2};
  int64_t t = 1;
  int32_t decided = 1;
  while (t < n - 2) {
    if (t + 2 > n_lags) { decided = 0; break; }
    if ((t % 2) == 1 && rho(t + 1) + rho(t + 2) < 0.) break;
    ++t;
  }
  // Decided: lags 1 .. t are summed; the last one read was t + 2 where the
  // rule fired and n - 1 where it ran to t = n - 2.  Undecided: every lag
  // given that the loop has passed.
  const int64_t last = decided ? t : (t < n_lags ? t : n_lags);
  std::vector<double> r(static_cast<size_t>(last));
  for (int64_t i = 1; i <= last; ++i) r[i - 1] = rho(i);
  // add.reduce starts from the first element and sums the rest pairwise
  double sum = last > 0 ? r[0] + np_pairwise_sum(r.data() + 1, last - 1) : 0.;
  if (sum < 0.) sum = 0.;
  int64_t lags = n_lags;
  if (decided) lags = (t < n - 2) ? t + 2 : n - 1;
  return {mn / (1. + 2. * sum), decided, lags};
}

}  // namespace rhmc_post
