// Host AddressSanitizer program for rhmc_dt_trials / rhmc_dt_trials_device
// (include/rhmc.h): the entry points' argument checks and error strings
// without a device.  Linked against the host-ASan objects of the library
// (`make -C hmc-stellar-toy-model_amd asan-dt`); tests/test_dt_host.py runs
// it.  Exit status 0 = every check passed and ASan reported nothing.
#include <cstdint>
#include <cstdio>
#include <cstring>

#include "rhmc.h"

static int g_fail = 0;
#define CHECK(cond)                                                              \
  do {                                                                           \
    if (!(cond)) {                                                               \
      std::fprintf(stderr, "FAIL %s:%d: %s [%s]\n", __FILE__, __LINE__, #cond,   \
                   rhmc_last_error());                                           \
      ++g_fail;                                                                  \
    }                                                                            \
  } while (0)

int main() {
  rhmc_params P;
  std::memset(&P, 0, sizeof(P));
  P.dt = 0.1;
  P.B_count = 24.98;
  P.fwhm_pix = 3.5;
  P.g_xx = P.g_ff = P.g_ff2 = P.g0 = P.g1 = P.g2 = 1.0;
  P.counter_max = 1000;
  rhmc_dt_opts o;
  std::memset(&o, 0, sizeof(o));
  o.n_iter = 2;
  o.grad = RHMC_DT_GRAD_REFERENCE;
  o.steps_min = 10;
  o.steps_max = 50;
  CHECK(sizeof(rhmc_dt_opts) == 6 * sizeof(int32_t));
  CHECK(sizeof(rhmc_dt_record) == 6 * sizeof(void*));
  constexpr int N = 2, NI = 2;
  double bg[4] = {1., 1., 1., 1.};                 // never read: no context
  int32_t bgi[N] = {0, 0};
  double q0[3 * N] = {100., 5., 5., 100., 9., 9.};
  double dt[3 * N] = {1., 0., 0., 1., .1, .1};
  int32_t fo[N] = {1, 0};
  double z[3 * N * NI] = {0};
  int32_t steps[N * NI] = {10, 11, 12, 13};
  double lnu[N * NI] = {-1., -1., -1., -1.};
  uint64_t sid[N] = {1, 2};
  int32_t nacc[N];
  rhmc_dt_record rec;
  std::memset(&rec, 0, sizeof(rec));

  auto says = [](const char* what) { return std::strstr(rhmc_last_error(), what) != nullptr; };
  auto host = [&](const rhmc_params* p, const rhmc_dt_opts* op, const double* b, int32_t nb,
                  const int32_t* bi, const double* q, const double* d, int64_t n,
                  const double* zz, const int32_t* st, const double* lu, const uint64_t* si) {
    return rhmc_dt_trials(nullptr, p, op, b, nb, bi, q, d, fo, n, zz, st, lu, 7, si, nacc, &rec);
  };
  auto dev = [&](const rhmc_params* p, const rhmc_dt_opts* op, const double* b, int32_t nb,
                 const int32_t* bi, const double* q, const double* d, int64_t n,
                 const double* zz, const int32_t* st, const double* lu, const uint64_t* si) {
    return rhmc_dt_trials_device(nullptr, p, op, b, nb, bi, q, d, fo, n, zz, st, lu, 7, si, nacc,
                                 nullptr, nullptr);
  };
  // everything in order but the context: host draws, device draws, both entries
  CHECK(host(&P, &o, bg, 1, bgi, q0, dt, N, z, steps, lnu, nullptr) == RHMC_ERR_ARG);
  CHECK(says("ctx is NULL"));
  CHECK(host(&P, &o, bg, 1, bgi, q0, dt, N, nullptr, nullptr, nullptr, sid) == RHMC_ERR_ARG);
  CHECK(says("ctx is NULL"));
  CHECK(dev(&P, &o, bg, 1, bgi, q0, dt, N, z, steps, lnu, nullptr) == RHMC_ERR_ARG);
  CHECK(says("ctx is NULL"));
  CHECK(host(&P, &o, bg, 1, bgi, q0, dt, 0, z, steps, lnu, nullptr) == RHMC_ERR_ARG);
  CHECK(says("ctx is NULL"));  // n = 0 is a no-op only on a context
  // the arguments are checked before the context is touched
  CHECK(host(nullptr, &o, bg, 1, bgi, q0, dt, N, z, steps, lnu, nullptr) == RHMC_ERR_ARG);
  CHECK(says("params is NULL"));
  CHECK(host(&P, nullptr, bg, 1, bgi, q0, dt, N, z, steps, lnu, nullptr) == RHMC_ERR_ARG);
  CHECK(says("opts is NULL"));
  CHECK(host(&P, &o, nullptr, 1, bgi, q0, dt, N, z, steps, lnu, nullptr) == RHMC_ERR_ARG);
  CHECK(says("bg is NULL"));
  CHECK(host(&P, &o, bg, 0, bgi, q0, dt, N, z, steps, lnu, nullptr) == RHMC_ERR_ARG);
  CHECK(says("n_bg"));
  CHECK(dev(&P, &o, bg, 1, nullptr, q0, dt, N, z, steps, lnu, nullptr) == RHMC_ERR_ARG);
  CHECK(says("bg_index is NULL"));
  CHECK(host(&P, &o, bg, 1, bgi, nullptr, dt, N, z, steps, lnu, nullptr) == RHMC_ERR_ARG);
  CHECK(says("q0 is NULL"));
  CHECK(dev(&P, &o, bg, 1, bgi, q0, nullptr, N, z, steps, lnu, nullptr) == RHMC_ERR_ARG);
  CHECK(says("dt is NULL"));
  CHECK(host(&P, &o, bg, 1, bgi, q0, dt, -1, z, steps, lnu, nullptr) == RHMC_ERR_ARG);
  CHECK(says("n < 0"));
  // n_iter outside 1..1024, an unknown gradient, reserved words
  rhmc_dt_opts b = o;
  for (int32_t ni : {0, -3, 1025}) {
    b.n_iter = ni;
    CHECK(host(&P, &b, bg, 1, bgi, q0, dt, N, nullptr, nullptr, nullptr, sid) == RHMC_ERR_ARG);
    CHECK(says("n_iter"));
    CHECK(dev(&P, &b, bg, 1, bgi, q0, dt, N, nullptr, nullptr, nullptr, sid) == RHMC_ERR_ARG);
    CHECK(says("n_iter"));
  }
  b = o;
  b.n_iter = 1024;                                 // the ends themselves are allowed
  CHECK(host(&P, &b, bg, 1, bgi, q0, dt, N, nullptr, nullptr, nullptr, sid) == RHMC_ERR_ARG);
  CHECK(says("ctx is NULL"));
  b = o;
  b.grad = 2;
  CHECK(host(&P, &b, bg, 1, bgi, q0, dt, N, z, steps, lnu, nullptr) == RHMC_ERR_ARG);
  CHECK(says("grad"));
  for (int i = 0; i < 2; ++i) {
    b = o;
    b.reserved[i] = 1;
    CHECK(host(&P, &b, bg, 1, bgi, q0, dt, N, z, steps, lnu, nullptr) == RHMC_ERR_ARG);
    CHECK(says("reserved"));
  }
  // only some of the three draw arrays
  CHECK(host(&P, &o, bg, 1, bgi, q0, dt, N, z, nullptr, nullptr, sid) == RHMC_ERR_ARG);
  CHECK(says("all three or none"));
  CHECK(host(&P, &o, bg, 1, bgi, q0, dt, N, z, steps, nullptr, sid) == RHMC_ERR_ARG);
  CHECK(says("all three or none"));
  CHECK(dev(&P, &o, bg, 1, bgi, q0, dt, N, nullptr, steps, lnu, sid) == RHMC_ERR_ARG);
  CHECK(says("all three or none"));
  // device draws need stream ids and a range of steps
  CHECK(host(&P, &o, bg, 1, bgi, q0, dt, N, nullptr, nullptr, nullptr, nullptr) == RHMC_ERR_ARG);
  CHECK(says("stream_id is NULL"));
  b = o;
  b.steps_max = b.steps_min;
  CHECK(host(&P, &b, bg, 1, bgi, q0, dt, N, nullptr, nullptr, nullptr, sid) == RHMC_ERR_ARG);
  CHECK(says("steps_min"));
  CHECK(host(&P, &b, bg, 1, bgi, q0, dt, N, z, steps, lnu, nullptr) == RHMC_ERR_ARG);
  CHECK(says("ctx is NULL"));  // the range is not read with host draws
  // host entry point: bg_index and steps out of range (the device one clamps)
  int32_t bad_bgi[N] = {0, 1};
  CHECK(host(&P, &o, bg, 1, bad_bgi, q0, dt, N, z, steps, lnu, nullptr) == RHMC_ERR_ARG);
  CHECK(says("bg_index[1]"));
  bad_bgi[1] = -1;
  CHECK(host(&P, &o, bg, 1, bad_bgi, q0, dt, N, z, steps, lnu, nullptr) == RHMC_ERR_ARG);
  CHECK(says("bg_index[1]"));
  CHECK(dev(&P, &o, bg, 1, bad_bgi, q0, dt, N, z, steps, lnu, nullptr) == RHMC_ERR_ARG);
  CHECK(says("ctx is NULL"));
  int32_t bad_steps[N * NI] = {10, 11, 65536, 13};
  CHECK(host(&P, &o, bg, 1, bgi, q0, dt, N, z, bad_steps, lnu, nullptr) == RHMC_ERR_ARG);
  CHECK(says("steps[2]"));
  bad_steps[2] = -1;
  CHECK(host(&P, &o, bg, 1, bgi, q0, dt, N, z, bad_steps, lnu, nullptr) == RHMC_ERR_ARG);
  CHECK(says("steps[2]"));
  bad_steps[2] = 65535;
  bad_steps[0] = 0;
  CHECK(host(&P, &o, bg, 1, bgi, q0, dt, N, z, bad_steps, lnu, nullptr) == RHMC_ERR_ARG);
  CHECK(says("ctx is NULL"));
  // the option is refused on a NULL context like every other
  CHECK(rhmc_ctx_set_option(nullptr, RHMC_OPT_DT_LANES, 64) == RHMC_ERR_ARG);
  int32_t v = 0;
  CHECK(rhmc_ctx_get_option(nullptr, RHMC_OPT_DT_LANES, &v) == RHMC_ERR_ARG);
  if (g_fail) return 1;
  std::printf("dt_asan: ok\n");
  return 0;
}
