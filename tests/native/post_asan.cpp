// Host AddressSanitizer program for librhmc_post's C-ABI (include/rhmc_post.h):
// every argument-error path and the host-only stopping rule rhmc_post_neff.
// It never creates a context, so it makes no HIP call and needs no GPU.
// Built by `make -C hmc-stellar-toy-model_amd/post asan`
// (tests/test_post_asan_host.py).
#include <cmath>
#include <cstdio>
#include <cstring>
#include <vector>

#include "rhmc_post.h"

static int g_fail = 0;

#define EXPECT(cond)                                                     \
  do {                                                                   \
    if (!(cond)) {                                                       \
      std::printf("FAILED line %d: %s  [%s]\n", __LINE__, #cond, rhmc_post_last_error()); \
      ++g_fail;                                                          \
    }                                                                    \
  } while (0)

static bool err_has(const char* word) { return std::strstr(rhmc_post_last_error(), word); }

int main() {
  EXPECT(rhmc_post_abi_version() == RHMC_POST_ABI_VERSION);
  EXPECT(sizeof(rhmc_post_layout) == 40 && sizeof(rhmc_post_detail) == 72);

  // fake non-NULL handles: every call below must fail before it touches them
  rhmc_post_ctx* ctx = reinterpret_cast<rhmc_post_ctx*>(0x1000);
  const double* dx = reinterpret_cast<const double*>(0x2000);
  std::vector<double> R(4), ne(4), V(64);
  const rhmc_post_layout ok = {40, 4, 3, 12, 3};

  auto conv = [&](rhmc_post_layout L, int64_t warm, int64_t thin, int64_t max_lag) {
    const int a = rhmc_post_convergence_device(ctx, dx, &L, warm, thin, max_lag, R.data(),
                                               ne.data(), nullptr, nullptr);
    const int b = rhmc_post_convergence(ctx, dx, &L, warm, thin, max_lag, R.data(), ne.data(),
                                        nullptr);
    return a == RHMC_POST_ERR_ARG && b == RHMC_POST_ERR_ARG;
  };
  rhmc_post_layout L = ok;
  L.n_chains = 1;  EXPECT(conv(L, 0, 1, 0) && err_has("n_chains"));
  L = ok; L.D = 0; EXPECT(conv(L, 0, 1, 0) && err_has("D must"));
  L = ok;          EXPECT(conv(L, 0, 0, 0) && err_has("thin"));
  EXPECT(conv(L, -1, 1, 0) && err_has("warm_up"));
  EXPECT(conv(L, 36, 1, 0) && err_has("n = 2"));
  EXPECT(conv(L, 0, 8, 0) && err_has("n = 2"));
  EXPECT(conv(L, 400, 1, 0) && err_has("n = 0"));
  EXPECT(conv(L, 0, 1, -1) && err_has("max_lag"));
  L.ld_iter = -12; EXPECT(conv(L, 0, 1, 0) && err_has("stride"));
  L = ok; L.ld_chain = -1; EXPECT(conv(L, 0, 1, 0) && err_has("stride"));
  L = ok; L.n_iter = 0; EXPECT(conv(L, 0, 1, 0));
  EXPECT(rhmc_post_convergence_device(ctx, dx, nullptr, 0, 1, 0, R.data(), ne.data(), nullptr,
                                      nullptr) == RHMC_POST_ERR_ARG);
  EXPECT(rhmc_post_convergence_device(nullptr, dx, &ok, 0, 1, 0, R.data(), ne.data(), nullptr,
                                      nullptr) == RHMC_POST_ERR_ARG && err_has("NULL"));
  EXPECT(rhmc_post_convergence_device(ctx, nullptr, &ok, 0, 1, 0, R.data(), ne.data(), nullptr,
                                      nullptr) == RHMC_POST_ERR_ARG);
  EXPECT(rhmc_post_convergence_device(ctx, dx, &ok, 0, 1, 0, nullptr, ne.data(), nullptr,
                                      nullptr) == RHMC_POST_ERR_ARG);
  EXPECT(rhmc_post_convergence(ctx, dx, &ok, 0, 1, 0, R.data(), nullptr, nullptr) ==
         RHMC_POST_ERR_ARG);

  // variogram: n = 20, lags 1 .. 19
  const int64_t bad_lags[][2] = {{0, 1}, {1, 0}, {20, 1}, {1, 20}, {19, 2}};
  for (auto& b : bad_lags)
    EXPECT(rhmc_post_variogram_device(ctx, dx, &ok, 0, 1, b[0], b[1], V.data(), nullptr) ==
               RHMC_POST_ERR_ARG && err_has("lags"));
  EXPECT(rhmc_post_variogram_device(ctx, dx, &ok, 0, 1, 1, 4, nullptr, nullptr) ==
         RHMC_POST_ERR_ARG);
  EXPECT(rhmc_post_variogram_device(nullptr, dx, &ok, 0, 1, 1, 4, V.data(), nullptr) ==
         RHMC_POST_ERR_ARG);

  // acceptance
  const int32_t* da = reinterpret_cast<const int32_t*>(0x3000);
  double* dr = reinterpret_cast<double*>(0x4000);
  const int64_t bad_win[][2] = {{-1, 5}, {0, -1}, {5, 5}, {6, 5}, {0, 41}, {-2, -2}, {-3, 10}};
  for (auto& w : bad_win) {
    EXPECT(rhmc_post_acceptance_device(ctx, da, 40, 4, 4, w[0], w[1], dr, nullptr) ==
               RHMC_POST_ERR_ARG && err_has("start"));
    EXPECT(rhmc_post_acceptance_fetch(ctx, da, 40, 4, 4, w[0], w[1], R.data(), nullptr) ==
               RHMC_POST_ERR_ARG && err_has("start"));
    EXPECT(rhmc_post_acceptance(ctx, da, 40, 4, 4, w[0], w[1], R.data()) == RHMC_POST_ERR_ARG);
  }
  EXPECT(rhmc_post_acceptance_device(ctx, da, 40, 4, -4, -1, -1, dr, nullptr) ==
         RHMC_POST_ERR_ARG && err_has("stride"));
  EXPECT(rhmc_post_acceptance_device(ctx, da, 0, 4, 4, -1, -1, dr, nullptr) == RHMC_POST_ERR_ARG);
  EXPECT(rhmc_post_acceptance_device(ctx, da, 40, 0, 4, -1, -1, dr, nullptr) == RHMC_POST_ERR_ARG);
  EXPECT(rhmc_post_acceptance_device(nullptr, da, 40, 4, 4, -1, -1, dr, nullptr) ==
         RHMC_POST_ERR_ARG);
  EXPECT(rhmc_post_acceptance_device(ctx, nullptr, 40, 4, 4, 3, 9, dr, nullptr) ==
         RHMC_POST_ERR_ARG);
  EXPECT(rhmc_post_acceptance_device(ctx, da, 40, 4, 4, -1, -1, nullptr, nullptr) ==
         RHMC_POST_ERR_ARG);
  EXPECT(rhmc_post_acceptance(nullptr, da, 40, 4, 4, -1, -1, R.data()) == RHMC_POST_ERR_ARG);
  EXPECT(rhmc_post_acceptance_fetch(ctx, da, 40, 4, 4, -1, -1, nullptr, nullptr) ==
         RHMC_POST_ERR_ARG);

  // options and creation arguments (no context is ever created)
  EXPECT(rhmc_post_set_option(nullptr, RHMC_POST_OPT_TBLK, 8) == RHMC_POST_ERR_ARG);
  EXPECT(rhmc_post_set_option(ctx, RHMC_POST_OPT_TBLK, 7) == RHMC_POST_ERR_ARG);
  EXPECT(rhmc_post_set_option(ctx, RHMC_POST_OPT_BLOCK, 100) == RHMC_POST_ERR_ARG);
  EXPECT(rhmc_post_set_option(ctx, 99, 1) == RHMC_POST_ERR_ARG);
  EXPECT(rhmc_post_create(0, nullptr) == RHMC_POST_ERR_ARG);
  rhmc_post_ctx* made = ctx;
  EXPECT(rhmc_post_create(-1, &made) == RHMC_POST_ERR_ARG && made == nullptr);
  rhmc_post_destroy(nullptr);

  // the stopping rule, with exactly-sized heap arrays so that a read past the
  // lags given is an ASan error
  double out = 0.;
  int32_t dec = -1;
  EXPECT(rhmc_post_neff(1, 10, 1., V.data(), 4, &out, &dec) == RHMC_POST_ERR_ARG);
  EXPECT(rhmc_post_neff(4, 2, 1., V.data(), 4, &out, &dec) == RHMC_POST_ERR_ARG);
  EXPECT(rhmc_post_neff(4, 10, 1., nullptr, 4, &out, &dec) == RHMC_POST_ERR_ARG);
  EXPECT(rhmc_post_neff(4, 10, 1., V.data(), -1, &out, &dec) == RHMC_POST_ERR_ARG);
  EXPECT(rhmc_post_neff(4, 10, 1., V.data(), 4, nullptr, &dec) == RHMC_POST_ERR_ARG);
  EXPECT(rhmc_post_neff(4, 10, 1., V.data(), 4, &out, nullptr) == RHMC_POST_ERR_ARG);

  for (int64_t n : {3, 4, 5, 12, 301}) {
    // rho_t = 0.9^t: positive and decaying, the rule runs to t = n - 2
    std::vector<double> rho(n - 1), Vt(n - 1);
    for (int64_t t = 1; t < n; ++t) {
      rho[t - 1] = std::pow(0.9, double(t));
      Vt[t - 1] = 2. * (1. - rho[t - 1]);
    }
    for (int64_t k = 0; k <= n - 1; ++k) {
      std::vector<double> part(Vt.begin(), Vt.begin() + k);   // exactly k lags
      EXPECT(rhmc_post_neff(6, n, 1., k ? part.data() : nullptr, k, &out, &dec) == RHMC_POST_OK);
      const bool need_all = n > 3;
      EXPECT(dec == ((need_all ? k == n - 1 : k >= 1) ? 1 : 0));
      EXPECT(std::isfinite(out));
    }
    double sum = 0.;
    for (int64_t t = 1; t <= n - 2; ++t) sum += rho[t - 1];
    EXPECT(rhmc_post_neff(6, n, 1., Vt.data(), n - 1, &out, &dec) == RHMC_POST_OK && dec == 1);
    EXPECT(std::fabs(out - 6. * n / (1. + 2. * sum)) <= 1e-12 * out);
    // more lags than exist (n_lags > n - 1) are not read
    EXPECT(rhmc_post_neff(6, n, 1., Vt.data(), n + 50, &out, &dec) == RHMC_POST_OK && dec == 1);
    // an alternating tail fires the rule early
    for (int64_t t = 2; t < n; ++t) Vt[t - 1] = 2. * (1. + 0.5);
    if (n > 3) {
      std::vector<double> part(Vt.begin(), Vt.begin() + 3);
      EXPECT(rhmc_post_neff(6, n, 1., part.data(), 3, &out, &dec) == RHMC_POST_OK && dec == 1);
      EXPECT(std::fabs(out - 6. * n / (1. + 2. * rho[0])) <= 1e-12 * out);
    }
    // rho_1 below 0.05 and a degenerate variance need one lag and none
    const double v1 = 2. * (1. - 0.01);
    EXPECT(rhmc_post_neff(6, n, 1., &v1, 1, &out, &dec) == RHMC_POST_OK && dec == 1 &&
           out == 6. * n);
    EXPECT(rhmc_post_neff(6, n, 0., nullptr, 0, &out, &dec) == RHMC_POST_OK && dec == 1 &&
           std::isnan(out));
  }

  if (g_fail) {
    std::printf("post asan: %d checks failed\n", g_fail);
    return 1;
  }
  std::printf("post asan ok\n");
  return 0;
}
