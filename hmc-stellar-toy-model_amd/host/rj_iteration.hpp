// rj_iteration.hpp — the steps of an iteration that the callback loop
// (rj_host.hpp) and the device-resident loop (rj_device.hpp) both take, each
// written once: the error message, a chain's stream start and end, the
// schedules, the first draws, the record rows, the accept decision, the
// recorded-V reuse, the phase clock and the launch plan by star count.
// A section of rhmc_rj.cpp's translation unit.
#pragma once

#include <chrono>
#include <cstdio>
#include <map>
#include <string>
#include <utility>

#include "rj_moves.hpp"

namespace {

thread_local std::string g_err;

int fail(int code, const std::string& msg) {
  g_err = msg;
  return code;
}

int engine_fail(int rc, const char* what) {
  const char* m = rhmc_last_error();
  return fail(rc, std::string("engine ") + what + " failed: " + (m ? m : ""));
}

// The diagnostic build (make timing: -DRHMC_RJ_TIMING) reports on stderr;
// the product build evaluates none of a trace's arguments.
#ifdef RHMC_RJ_TIMING
#define RJ_TRACE(...) std::fprintf(stderr, __VA_ARGS__)
#else
#define RJ_TRACE(...) ((void)0)
#endif
struct Stopwatch {
  std::chrono::steady_clock::time_point t0 = std::chrono::steady_clock::now();
  double ms() const {
    return std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count() * 1e3;
  }
};

// ------------------------------------------------------------- a chain's stream
// chain c of a part that starts at the caller's chain rec_off: np.random.seed
// (seeds[c]), or the caller's saved state
void start_stream(Chain& h, const rhmc_rj_config* cfg, const uint32_t* seeds, int64_t rec_off,
                  int64_t c) {
  if (cfg->use_states) {
    const rhmc_np_state& st = cfg->states[rec_off + c];
    h.rng.set_state(st.key, st.pos, st.has_gauss, st.gauss);
  } else {
    h.rng.seed(seeds[c]);
  }
}

// the end of the run for chain c: its final row (src's 3 K values, zeros to
// zero_to), star count and stream go back to the caller
void finish_chain(const Chain& h, const rhmc_rj_config* cfg, int64_t rec_off, int64_t c,
                  const double* src, int64_t zero_to, int64_t W, double* q, int32_t* K) {
  put_row(q + c * W, src, 3 * (int64_t)h.K, zero_to, W);
  _mm_sfence();
  K[c] = h.K;
  if (cfg->states) {
    rhmc_np_state& st = cfg->states[rec_off + c];
    h.rng.get_state(st.key, &st.pos, &st.has_gauss, &st.gauss);
  }
}

// g_ff2 / beta of iteration l (:1010-1016)
void apply_schedules(const rhmc_rj_config* cfg, int64_t l, rhmc_params& P) {
  if (cfg->n_g_ff2 > 0) P.g_ff2 = cfg->schedule_g_ff2[std::min<int64_t>(l, cfg->n_g_ff2 - 1)];
  if (cfg->n_beta > 0) P.beta = cfg->schedule_beta[std::min<int64_t>(l, cfg->n_beta - 1)];
}

// an iteration's first draws (:1021-1022, :1031-1033): z = randn(3K), the
// move type, grow / shrink
void draw_start(Chain& h, const rhmc_rj_config* cfg, double* z) {
  for (int64_t i = 0; i < 3 * (int64_t)h.K; ++i) z[i] = h.rng.gauss();
  h.move = (int)choice(h.rng, cfg->P_move, 3, h.cdf);
  h.grow = false;
  if (h.move != 0) {
    const double half[2] = {0.5, 0.5};
    h.grow = choice(h.rng, half, 2, h.cdf) == 0;  // [True, False]
  }
}

// ------------------------------------------------------------------ records
// rhmc_rj_record::move
enum MoveCode : int32_t { kWithin = 0, kBirth = 1, kDeath = 2, kSplit = 3, kMerge = 4 };

MoveCode move_code(int move, bool grow) {
  if (move == 0) return kWithin;
  return move == 1 ? (grow ? kBirth : kDeath) : (grow ? kSplit : kMerge);
}

// record row r, the state at the start of an iteration: q and p (3 K values
// each, zero-padded to 3 N_max; n_stars[r] is read before it is rewritten),
// the energies, the star count and the move
void record_start(const rhmc_rj_config* cfg, const rhmc_rj_record* rec, int64_t r, int64_t W,
                  const double* q, const double* p, int32_t K, double V0, double T0, double E0,
                  int move, bool grow) {
  if (!rec) return;
  const int64_t d = 3 * (int64_t)K, zt = zero_end(cfg, rec, r, d, W);
  if (rec->q_chain) put_row(rec->q_chain + r * W, q, d, zt, W);
  if (rec->p_chain) put_row(rec->p_chain + r * W, p, d, zt, W);
  _mm_sfence();
  if (rec->V_chain) rec->V_chain[r] = V0;
  if (rec->T_chain) rec->T_chain[r] = T0;
  if (rec->E_chain) rec->E_chain[r] = E0;
  if (rec->n_stars) rec->n_stars[r] = K;
  if (rec->move) rec->move[r] = move_code(move, grow);
}

// the Metropolis decision (:1072-1083 within the model, :1120-1131 for a
// jump with its ln-acceptance factor); u = ln(uniform)
bool accepts(int move, double E0, double E1, double u, double factor) {
  if (move == 0) {
    const double dE = E1 - E0;
    return (dE < 0) || (u < -dE);
  }
  const double ln_alpha0 = -(E1 - E0) + factor;
  return (ln_alpha0 > 0) || (u < ln_alpha0);
}

void record_accept(const rhmc_rj_record* rec, int64_t r, bool acc, bool dead) {
  if (!rec) return;
  if (rec->accept) rec->accept[r] = acc ? 1 : 0;
  if (rec->flags) rec->flags[r] = dead ? (int32_t)RHMC_RJ_DEAD_END : 0;
}

// V of every chain's q at the end of the previous iteration (V(q') if it
// accepted, else its V(q)) and the prior parameters it was computed with:
// while a schedule leaves them unchanged, an iteration's V(q) is that value
// (the engine's V of a chain does not depend on the batch it is in:
// tests/test_gpu_rj_native.py recomputes every recorded V), saving one
// engine phase per iteration
struct RecordedV {
  std::vector<double> V;
  double g_ff2 = 0., beta = 0.;
  bool ok = false;
  explicit RecordedV(int64_t n) : V((size_t)n) {}
  bool valid(const rhmc_params& P) const { return ok && P.g_ff2 == g_ff2 && P.beta == beta; }
  void store(const rhmc_params& P) {  // V is this iteration's, computed with P
    g_ff2 = P.g_ff2;
    beta = P.beta;
    ok = true;
  }
};

// The wall time of a loop's phases (rhmc_rj_record::phase_s).
struct PhaseClock {
  double phase[7] = {0, 0, 0, 0, 0, 0, 0};
  std::chrono::steady_clock::time_point clk = std::chrono::steady_clock::now();
  int64_t l = 0;  // the iteration, for the diagnostic build
  void lap(int i) {  // the time since the last lap goes to phase i
    const auto t = std::chrono::steady_clock::now();
    const double dt = std::chrono::duration<double>(t - clk).count();
    phase[i] += dt;
    clk = t;
    if (dt > 1e-3) RJ_TRACE("rj slow phase %d: %.3f ms (l %lld)\n", i, dt * 1e3, (long long)l);
  }
  void add_to(double* out) const {
    if (out)
      for (int i = 0; i < 7; ++i) out[i] += phase[i];
  }
};

// -------------------------------------------------------------- launch plan
// One phase's launch plan over chains `idx` (star counts K): the chains of the
// slotted kernels' star counts grouped by register slots (one ragged launch
// each), then one packed launch per other star count (first appearance).
struct Call {
  bool ragged;
  int32_t Kmin, Kmax;
  int64_t off, n;  // the call's chains: order[off .. off + n)
};
struct Plan {
  std::vector<int64_t> order;
  std::vector<Call> calls;
};

// The engine's ragged launch class of k stars: one kernel family and one
// register-slot count each, the slot ranges documented for rhmc_ragged_ok in
// include/rhmc.h (2-10 stars: the pixel-major kernel on 32/48-px images; then
// the slot counts of the dense / windowed kernels)
constexpr int kSlotClasses = 6;
int slot_class(int32_t k) {
  if (k <= 10) return 0;
  if (k <= 64) return 1;
  if (k <= 128) return 2;
  if (k <= 256) return 3;
  return k <= 512 ? 4 : 5;
}

// ragged_ok[k]: the engine serves k stars with a ragged launch (all zero: one
// packed call per star count, the callback loop's grouping)
Plan make_plan(const std::vector<int64_t>& idx, const std::vector<int32_t>& K,
               const std::vector<char>& ragged_ok) {
  Plan pl;
  std::vector<int64_t> cls[kSlotClasses];
  std::vector<std::pair<int32_t, std::vector<int64_t>>> groups;
  std::map<int32_t, size_t> where;
  for (int64_t c : idx) {
    const int32_t k = K[c];
    if (ragged_ok[k]) {
      cls[slot_class(k)].push_back(c);
      continue;
    }
    auto it = where.find(k);
    if (it == where.end()) {
      where[k] = groups.size();
      groups.push_back({k, {c}});
    } else {
      groups[it->second].second.push_back(c);
    }
  }
  for (auto& v : cls) {
    if (v.empty()) continue;
    int32_t lo = 1024, hi = 1;
    for (int64_t c : v) {
      lo = std::min(lo, K[c]);
      hi = std::max(hi, K[c]);
    }
    pl.calls.push_back({true, lo, hi, (int64_t)pl.order.size(), (int64_t)v.size()});
    pl.order.insert(pl.order.end(), v.begin(), v.end());
  }
  for (auto& g : groups) {
    pl.calls.push_back({false, g.first, g.first, (int64_t)pl.order.size(),
                        (int64_t)g.second.size()});
    pl.order.insert(pl.order.end(), g.second.begin(), g.second.end());
  }
  return pl;
}

// launch() -> rc; the diagnostic build reports a launch call that blocks
template <class F>
int timed_launch(const char* what, const Call& c, F launch) {
#ifdef RHMC_RJ_TIMING
  const Stopwatch sw;
  const int rc = launch();
  const double ms = sw.ms();
  if (ms > 0.2)
    RJ_TRACE("rj slow launch: %s K %d-%d n %lld %.3f ms\n", what, c.Kmin, c.Kmax, (long long)c.n,
             ms);
  return rc;
#else
  (void)what;
  (void)c;
  return launch();
#endif
}

}  // namespace
