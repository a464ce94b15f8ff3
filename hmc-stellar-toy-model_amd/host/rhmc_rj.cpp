// rhmc_rj.cpp — librhmc_rj.so: multi_gym.run_RHMC's reversible-jump sampler
// (sampler_RHMC.py:937-1198, moves :1200-1445) for many chains at once, native
// host code around the engine's C-ABI (include/rhmc_rj.h).
//
// One iteration l (every chain c has its own RandomState replica and star
// count K_c):
//   1. host, per chain, in parallel: g_ff2 / beta from the schedules
//      (:1010-1016), H(q) (:229-258), p = randn(3K) sqrt(H) (:1021-1022),
//      T0 (:1026), the move type (:1045) and grow / shrink (:1094, :1140)
//   2. engine: V(q) of every chain, grouped by K                  (:1025)
//   3. engine: Nsteps steps on every chain, grouped by K     (:1053, :1098)
//   4. host, jumping chains: p = -p, the proposal and its ln-acceptance
//      factor (:1099-1102; birth_death_move / split_merge_move)
//   5. engine: Nsteps steps on the jumping chains at their new K   (:1109)
//   6. engine: V(q') of every chain                          (:1069, :1117)
//   7. host: E1 = V' + T(p', H(q')), the accept uniform, accept / restore
//      (:1072-1083, :1120-1131)
// The host expressions follow the reference's operation order
// (rhmc_amd/sampler.py's _H_vec / T / moves, which tests pin to it).
//
// One translation unit (inlining and -ffp-contract=off rounding as one file);
// the headers are its sections, one role each:
//   rj_model.hpp      record rows; the metric, T, choice, the Beta density
//   rj_pool.hpp       the fork-join thread pool and the process's pools
//   rj_moves.hpp      a chain's host state; birth/death, split/merge
//   rj_iteration.hpp  the steps both loops take, written once
//   rj_host.hpp       the callback loop        (rhmc_rj_run_physics)
//   rj_device.hpp     the device-resident loop (rhmc_rj_run), its buffers
//   rj_registry.hpp   the owner of the per-(device, pipe) buffers
// and this file: the argument checks, the fan-out over pipes and the C-ABI.
#include "rhmc_rj.h"

#include <array>

#include "rj_device.hpp"
#include "rj_host.hpp"
#include "rj_registry.hpp"

namespace {

constexpr int kMaxPipes = 8;  // rhmc_rj_config::n_pipes

int check(const rhmc_params* P, const rhmc_rj_config* cfg, const double* q, const int32_t* K,
          const uint32_t* seeds, int64_t n, const rhmc_rj_record* rec) {
  if (!P || !cfg) return fail(RHMC_ERR_ARG, "params or config is NULL");
  if (cfg->records_zero_padded < 0 || cfg->records_zero_padded > 3)
    return fail(RHMC_ERR_ARG, "records_zero_padded must be in [0, 3]");
  if (cfg->n_pipes < 0 || cfg->n_pipes > kMaxPipes)
    return fail(RHMC_ERR_ARG, "n_pipes must be in [0, 8]");
  if (n < 0) return fail(RHMC_ERR_ARG, "n < 0");
  if (n > 0 && (!q || !K)) return fail(RHMC_ERR_ARG, "q or K is NULL");
  if (cfg->use_states != 0 && cfg->use_states != 1)
    return fail(RHMC_ERR_ARG, "use_states must be 0 or 1");
  if (n > 0 && cfg->use_states && !cfg->states)
    return fail(RHMC_ERR_ARG, "use_states without states");
  if (n > 0 && !cfg->use_states && !seeds) return fail(RHMC_ERR_ARG, "seeds is NULL");
  for (int64_t c = 0; cfg->use_states && c < n; ++c)
    if (cfg->states[c].pos < 0 || cfg->states[c].pos > 624)
      return fail(RHMC_ERR_ARG, "states[c].pos must be in [0, 624]");
  if (cfg->n_iter < 0 || cfg->n_steps < 0) return fail(RHMC_ERR_ARG, "n_iter or n_steps < 0");
  if (cfg->N_max < 1 || cfg->N_max > 1024)
    return fail(RHMC_ERR_ARG, "N_max must be in [1, 1024]");
  if (cfg->rows < 3 || cfg->cols < 3) return fail(RHMC_ERR_ARG, "rows / cols < 3");
  if ((cfg->n_g_ff2 > 0 && !cfg->schedule_g_ff2) || (cfg->n_beta > 0 && !cfg->schedule_beta) ||
      cfg->n_g_ff2 < 0 || cfg->n_beta < 0)
    return fail(RHMC_ERR_ARG, "schedule array missing");
  double ps = 0.;
  for (int i = 0; i < 3; ++i) {
    if (!(cfg->P_move[i] >= 0.0)) return fail(RHMC_ERR_ARG, "P_move entries must be >= 0");
    ps += cfg->P_move[i];
  }
  if (!(std::fabs(ps - 1.0) <= 1.4901161193847656e-08))  // choice(): sqrt(eps) tolerance
    return fail(RHMC_ERR_ARG, "P_move must sum to 1");
  if ((cfg->P_move[1] > 0 || cfg->P_move[2] > 0) &&
      !(cfg->fmin > 0 && cfg->fmax > 0 && cfg->K_split > 0 && cfg->beta_a > 0 && cfg->beta_b > 0))
    return fail(RHMC_ERR_ARG, "jumps need fmin, fmax, K_split, beta_a, beta_b > 0");
  for (int64_t c = 0; c < n; ++c)
    if (K[c] < 1 || K[c] > cfg->N_max) return fail(RHMC_ERR_ARG, "K[c] must be in [1, N_max]");
  if ((cfg->records_zero_padded & RHMC_RJ_ZP_RECORDS) && !(rec && rec->n_stars))
    return fail(RHMC_ERR_ARG, "records_zero_padded needs the n_stars record");
  return 0;
}

int host_threads(const rhmc_rj_config* cfg) {
  const int nt = cfg->n_threads;
  if (nt > 0) return nt;
  return (int)std::min<unsigned>(16u, std::max(1u, std::thread::hardware_concurrency()));
}

// Split n chains into `pipes` contiguous parts run concurrently, part i on
// its own host thread (part 0 on the caller's), all on one shared pool of
// nt - pipes workers: body(i, first chain, count, pool, phase[7]) -> rc.  The
// first failing part's error is the one reported.
template <class Body>
int run_pipes(int pipes, int64_t n, int nt, double* phase, Body body) {
  const std::shared_ptr<Pool> pool = shared_pool(std::max(0, nt - std::max(1, pipes)));
  // one part's body on this thread; an exception becomes an error code (no
  // C++ exception may cross the ABI, and none may leave a std::thread)
  auto guarded = [&](int i, int64_t f, int64_t m, double* ph, std::string& err) {
    try {
      const int rc = body(i, f, m, pool.get(), ph);
      if (rc) err = g_err;
      return rc;
    } catch (const std::exception& e) {
      err = std::string("host exception: ") + e.what();
    } catch (...) {
      err = "host exception";
    }
    return (int)RHMC_ERR_NOMEM;
  };
  if (pipes <= 1) {
    std::string err;
    const int rc = guarded(0, 0, n, phase, err);
    if (rc) g_err = err;
    return rc;
  }
  std::vector<int64_t> first((size_t)pipes + 1);
  for (int i = 0; i <= pipes; ++i) first[i] = n * i / pipes;
  std::vector<std::array<double, 7>> ph((size_t)pipes);
  std::vector<int> rcs((size_t)pipes, 0);
  std::vector<std::string> errs((size_t)pipes);
  std::vector<std::thread> ts;
  ts.reserve((size_t)pipes);
  for (int i = 1; i < pipes; ++i) {
    ph[i].fill(0.);
    try {
      ts.emplace_back([&, i] {
        rcs[i] = guarded(i, first[i], first[i + 1] - first[i], ph[i].data(), errs[i]);
      });
    } catch (const std::exception& e) {  // this part does not run: report it
      rcs[i] = RHMC_ERR_NOMEM;
      errs[i] = std::string("cannot start a pipe thread: ") + e.what();
    }
  }
  ph[0].fill(0.);
  rcs[0] = guarded(0, first[0], first[1] - first[0], ph[0].data(), errs[0]);
  for (auto& t : ts) t.join();
  for (int i = 0; i < pipes; ++i)
    for (int k = 0; k < 7; ++k) phase[k] += ph[i][k];
  for (int i = 0; i < pipes; ++i)
    if (rcs[i]) {
      g_err = errs[i];
      return rcs[i];
    }
  return 0;
}

int pipes_for(const rhmc_rj_config* cfg, int64_t n) {
  // default for the device-resident driver, measured at big-sim4 geometry
  // (profiles/r05_pipes/, three repeats on one box, chain-steps/s): 4,096
  // chains 1.70e7 / 1.82e7 / 1.84e7 with 2 / 3 / 4 pipes; 16,384 chains
  // 1.80e7 / 2.06e7 / 2.12e7.  After the ragged pixel-major launches
  // (profiles/r05_pipes2/, r05_pipes3/, four repeats): 4,096 chains B4 2.62e7 /
  // 2.72e7 with 3 / 4 pipes, the flagship 2.64e7 / 2.78e7; 6 and 8 pipes
  // (more streams than the box's 4 hardware queues) 0.75-0.95x.  At 16,384
  // chains 8 pipes beat 4 (profiles/r05_pipes8/, two repeats): B4 3.28e7 /
  // 3.18e7 against 2.94e7 / 2.82e7 (4,096 chains: 0.6x)
  int pipes = cfg->n_pipes > 0
                  ? cfg->n_pipes
                  : (n >= 16384 ? 8 : n >= 4096 ? 4 : n >= 2048 ? 3 : n >= 1024 ? 2 : 1);
  return (int)std::max<int64_t>(1, std::min<int64_t>(pipes, n));
}

// The pipes' buffers and streams by (device, pipe index).  Never destroyed:
// at process exit the HIP runtime may be gone before static destructors run
// (rhmc_rj_release is the way to free them).
rj::Registry<Work>& works() {
  static auto* r = new rj::Registry<Work>();
  return *r;
}

}  // namespace

extern "C" {

int rhmc_rj_run_physics(const rhmc_rj_physics* phys, const rhmc_params* P,
                        const rhmc_rj_config* cfg, double* q, int32_t* K, const uint32_t* seeds,
                        int64_t n, const rhmc_rj_record* rec) {
  try {
    if (int rc = check(P, cfg, q, K, seeds, n, rec)) return rc;
    double phase[7] = {0, 0, 0, 0, 0, 0, 0};
    const int nt = host_threads(cfg);
    // with pipes > 1 the callbacks are called from that many threads at once
    const int64_t W = 3 * (int64_t)cfg->N_max;
    int rc = run_pipes(cfg->n_pipes > 1 ? pipes_for(cfg, n) : 1, n, nt, phase,
                       [&](int, int64_t f, int64_t m, Pool* pool, double* ph) {
                         return run(phys, P, cfg, q + f * W, K + f,
                                    seeds ? seeds + f : nullptr, m, rec, n, f, pool, ph);
                       });
    if (rc == 0 && rec && rec->phase_s) std::copy(phase, phase + 7, rec->phase_s);
    return rc;
  } catch (const std::exception& e) {
    return fail(RHMC_ERR_NOMEM, std::string("host exception: ") + e.what());
  }
}

int rhmc_rj_run(rhmc_ctx* ctx, const rhmc_params* P, const rhmc_rj_config* cfg, double* q,
                int32_t* K, const uint32_t* seeds, int64_t n, const rhmc_rj_record* rec) {
  if (!ctx) return fail(RHMC_ERR_ARG, "ctx is NULL");
  const Stopwatch sw;  // diagnostic build: when the pipes start and return
  try {
    if (int rc = check(P, cfg, q, K, seeds, n, rec)) return rc;
    const double* dimg = nullptr;
    if (int rc = rhmc_ctx_image_device(ctx, &dimg)) return rc;
    if (!dimg) return fail(RHMC_ERR_ARG, "context has no image");
    hipPointerAttribute_t at;
    RJ_HIP(hipPointerGetAttributes(&at, dimg));
    const int dev = at.device;
    DeviceGuard guard;  // the caller's device comes back on return, after the leases go
    RJ_HIP(hipSetDevice(dev));
    const int pipes = pipes_for(cfg, n);
    const int nt = host_threads(cfg);
    // each pipe on its own kept buffers and streams, held for the run
    auto work = works().acquire(dev, pipes);
    const int64_t W = 3 * (int64_t)cfg->N_max;
    double phase[7] = {0, 0, 0, 0, 0, 0, 0};
    RJ_TRACE("rj run: pipes start at %.3f ms\n", sw.ms());
    const int rc = run_pipes(pipes, n, nt, phase, [&](int i, int64_t f, int64_t m, Pool* pool,
                                                      double* ph) {
      RJ_TRACE("rj run: pipe %d starts at %.3f ms\n", i, sw.ms());
      if (hipSetDevice(dev) != hipSuccess) return fail(RHMC_ERR_HIP, "hipSetDevice failed");
      const int rc_i = run_device(ctx, dev, &work[i], P, cfg, q + f * W, K + f,
                                  seeds ? seeds + f : nullptr, m, rec, n, f, pool, ph);
      RJ_TRACE("rj run: pipe %d returns at %.3f ms\n", i, sw.ms());
      return rc_i;
    });
    RJ_TRACE("rj run: pipes joined at %.3f ms\n", sw.ms());
    if (rc == 0 && rec && rec->phase_s) std::copy(phase, phase + 7, rec->phase_s);
    return rc;
  } catch (const std::exception& e) {
    return fail(RHMC_ERR_NOMEM, std::string("host exception: ") + e.what());
  }
}

int rhmc_rj_release(int32_t device) {
  try {
    DeviceGuard guard;
    works().release(device);  // a run using a pipe's buffers finishes first
    drop_idle_pools();
    return 0;
  } catch (const std::exception& e) {
    return fail(RHMC_ERR_NOMEM, std::string("host exception: ") + e.what());
  }
}

int rhmc_np_draws(uint32_t seed, int32_t kind, double a, double b, int64_t n, double* out) {
  if (n < 0 || (n > 0 && !out)) return fail(RHMC_ERR_ARG, "bad n or out");
  rhmc_np::Legacy r(seed);
  for (int64_t i = 0; i < n; ++i) {
    switch (kind) {
      case 0: out[i] = r.random_sample(); break;
      case 1: out[i] = r.gauss(); break;
      case 2:
        if (!(a >= 1.0)) return fail(RHMC_ERR_ARG, "randint needs a >= 1");
        out[i] = (double)r.randint(0, (int64_t)a);
        break;
      case 3: out[i] = r.beta(a, b); break;
      case 4: out[i] = r.standard_gamma(a); break;
      case 5: out[i] = r.standard_exponential(); break;
      default: return fail(RHMC_ERR_ARG, "unknown kind");
    }
  }
  return 0;
}

int rhmc_rj_pack_starts(const double* rows, const int32_t* K, int64_t n, int32_t N_max,
                        double flux_to_count, double* q) {
  return rhmc_rj_pack_starts_padded(rows, K, n, N_max, flux_to_count, q, nullptr);
}

int rhmc_rj_pack_starts_padded(const double* rows, const int32_t* K, int64_t n, int32_t N_max,
                               double flux_to_count, double* q, const int32_t* K_prev) {
  if (n < 0 || N_max < 1) return fail(RHMC_ERR_ARG, "bad n or N_max");
  if (n > 0 && (!rows || !K || !q)) return fail(RHMC_ERR_ARG, "rows, K or q is NULL");
  const int64_t W = 3 * (int64_t)N_max;
  std::vector<int64_t> at;
  try {
    at.resize((size_t)n + 1);
  } catch (...) {
    return fail(RHMC_ERR_NOMEM, "pack_starts: out of host memory");
  }
  at[0] = 0;
  for (int64_t c = 0; c < n; ++c) {
    if (K[c] < 1 || K[c] > N_max) return fail(RHMC_ERR_ARG, "K[c] must be in [1, N_max]");
    at[c + 1] = at[c] + 3 * (int64_t)K[c];
  }
  auto pack = [&](int64_t c0, int64_t c1) {
    std::vector<double> tmp((size_t)W);
    // pow is a pure function: a small direct-mapped memo of magnitudes (the
    // flagship starts every chain from the same model stars)
    uint64_t memo_key[64];
    double memo_val[64];
    bool memo_ok[64] = {};
    for (int64_t c = c0; c < c1; ++c) {
      const double* src = rows + at[c];
      for (int32_t k = 0; k < K[c]; ++k) {
        const double v = src[3 * k];
        // mag2flux_converter (sampler_RHMC.py:147-152, utils.py:24-25): libm pow,
        // the function NumPy's and Python's float power call
        double f = v;
        if (flux_to_count > 0) {
          uint64_t bits;
          std::memcpy(&bits, &v, 8);
          const int slot = (int)((bits * 0x9E3779B97F4A7C15ull) >> 58);
          if (!memo_ok[slot] || memo_key[slot] != bits) {
            memo_key[slot] = bits;
            memo_val[slot] = std::pow(10.0, 0.4 * (22.5 - v));
            memo_ok[slot] = true;
          }
          f = memo_val[slot] * flux_to_count;
        }
        tmp[3 * k] = f;
        tmp[3 * k + 1] = src[3 * k + 1];
        tmp[3 * k + 2] = src[3 * k + 2];
      }
      // zero-padded (streamed), or only up to the row's old width
      const int64_t d = 3 * (int64_t)K[c];
      const int32_t kp = K_prev ? K_prev[c] : 0;
      put_row(q + c * W, tmp.data(), d, kp >= 1 && kp <= N_max ? std::max(d, 3 * (int64_t)kp) : W,
              W);
    }
    _mm_sfence();
  };
  // a few host threads for large batches (one pow per distinct magnitude, a
  // 3 N_max row of stores per chain); chains split in contiguous ranges, so
  // the result does not depend on the thread count
  const int64_t work = at[n];
  const int nt = (int)std::min<int64_t>(8, std::max<int64_t>(1, work / 60000));
  std::vector<std::thread> th;
  for (int t = 1; t < nt; ++t) {
    const int64_t c0 = n * t / nt, c1 = n * (t + 1) / nt;
    try {
      th.emplace_back(pack, c0, c1);
    } catch (...) {  // no thread: this thread packs the range
      pack(c0, c1);
    }
  }
  pack(0, nt > 1 ? n / nt : n);
  for (auto& t : th) t.join();
  return 0;
}

int rhmc_rj_beta_eval(double a, double b, const double* x, int64_t n, double* pdf, double* logpdf) {
  if (!(a > 0) || !(b > 0)) return fail(RHMC_ERR_ARG, "beta_a and beta_b must be > 0");
  if (n < 0 || (n > 0 && !x)) return fail(RHMC_ERR_ARG, "bad n or x");
  BetaDist d;
  d.set(a, b);
  for (int64_t i = 0; i < n; ++i) {
    if (pdf) pdf[i] = d.pdf(x[i]);
    if (logpdf) logpdf[i] = d.logpdf(x[i]);
  }
  return 0;
}

const char* rhmc_rj_last_error(void) { return g_err.c_str(); }

}  // extern "C"
