// rj_host.hpp — rhmc_rj_run_physics' loop: the iteration on host arrays
// around the caller's engine callbacks, one call per distinct star count and
// phase.  A section of rhmc_rj.cpp's translation unit.
#pragma once

#include <cstring>

#include "rj_iteration.hpp"
#include "rj_pool.hpp"

namespace {

struct HostRun {
  const rhmc_rj_physics* phys;
  Moves mv;
  std::vector<Chain> ch;
  std::vector<int32_t> Kv;             // the chains' star counts, for the plans
  const std::vector<char> no_ragged;   // every star count is one packed call

  HostRun(const rhmc_rj_physics* ph, const rhmc_params* P0, const rhmc_rj_config* cfg, int64_t n)
      : phys(ph), mv(P0, cfg), ch((size_t)n), Kv((size_t)n), no_ragged((size_t)cfg->N_max + 1, 0) {}

  // chains idx grouped by star count in order of first appearance
  Plan plan(const std::vector<int64_t>& idx) {
    for (int64_t c : idx) Kv[c] = ch[c].K;
    return make_plan(idx, Kv, no_ragged);
  }

  int energies(const std::vector<int64_t>& idx, std::vector<double>& V) {
    std::vector<double> qb, vb;
    const Plan pl = plan(idx);
    for (const Call& grp : pl.calls) {
      const int32_t K = grp.Kmin;
      const int64_t* cs = &pl.order[grp.off];
      const size_t d = 3 * (size_t)K, m = (size_t)grp.n;
      qb.resize(m * d);
      vb.assign(m, 0.);
      for (size_t i = 0; i < m; ++i) std::memcpy(&qb[i * d], ch[cs[i]].q.data(), d * 8);
      const int rc = phys->energy(phys->user, &mv.P, qb.data(), grp.n, K, mv.cfg->f_pos, vb.data());
      if (rc != 0) return engine_fail(rc, "energy");
      for (size_t i = 0; i < m; ++i) V[cs[i]] = vb[i];
    }
    return 0;
  }

  int trajectories(const std::vector<int64_t>& idx) {
    std::vector<double> qb, pb;
    const Plan pl = plan(idx);
    for (const Call& grp : pl.calls) {
      const int32_t K = grp.Kmin;
      const int64_t* cs = &pl.order[grp.off];
      const size_t d = 3 * (size_t)K, m = (size_t)grp.n;
      qb.resize(m * d);
      pb.resize(m * d);
      for (size_t i = 0; i < m; ++i) {
        std::memcpy(&qb[i * d], ch[cs[i]].q.data(), d * 8);
        std::memcpy(&pb[i * d], ch[cs[i]].p.data(), d * 8);
      }
      const int rc = phys->steps(phys->user, &mv.P, qb.data(), pb.data(), grp.n, K,
                                 mv.cfg->n_steps);
      if (rc != 0) return engine_fail(rc, "steps");
      for (size_t i = 0; i < m; ++i) {
        std::memcpy(ch[cs[i]].q.data(), &qb[i * d], d * 8);
        std::memcpy(ch[cs[i]].p.data(), &pb[i * d], d * 8);
      }
    }
    return 0;
  }
};

// n chains (a contiguous slice of the caller's: q, K, seeds point at its
// first chain); record row l of chain c is l * rec_stride + rec_off + c; the
// host work on `pool`; the phase times are added to phase_out[7].
int run(const rhmc_rj_physics* phys, const rhmc_params* P0,
        const rhmc_rj_config* cfg, double* q, int32_t* K, const uint32_t* seeds, int64_t n,
        const rhmc_rj_record* rec, int64_t rec_stride, int64_t rec_off, Pool* pool,
        double* phase_out) {
  if (!phys || !phys->energy || !phys->steps) return fail(RHMC_ERR_ARG, "physics is NULL");
  HostRun R(phys, P0, cfg, n);
  const int64_t W = 3 * (int64_t)cfg->N_max;
  std::vector<int64_t> all((size_t)n);
  for (int64_t c = 0; c < n; ++c) {
    all[c] = c;
    Chain& h = R.ch[c];
    start_stream(h, cfg, seeds, rec_off, c);
    h.K = K[c];
    h.q.assign(q + c * W, q + c * W + 3 * (int64_t)K[c]);
  }
  const int64_t rows_n = (int64_t)cfg->n_iter + 1;
  std::vector<double> V0((size_t)n), V1((size_t)n), T0((size_t)n);
  RecordedV V_end(n);
  PhaseClock clock;
  for (int64_t l = 0; l < rows_n; ++l) {
    clock.l = l;
    apply_schedules(cfg, l, R.mv.P);
    const Metric M = R.mv.metric();
    // 1. momentum, T0, move type, grow / shrink
    parallel(pool, all, [&](int64_t c) {
      Chain& h = R.ch[c];
      const int64_t d = 3 * (int64_t)h.K;
      h.H.resize((size_t)d);
      M.all(h.q.data(), d, h.H.data());
      h.p.resize((size_t)d);
      draw_start(h, cfg, h.p.data());       // z = randn(3K), then the move
      for (int64_t i = 0; i < d; i += 3) {  // p = z * sqrt(H); H_y = H_x
        const double sf = std::sqrt(h.H[i]), sx = std::sqrt(h.H[i + 1]);
        h.p[i] = h.p[i] * sf;
        h.p[i + 1] = h.p[i + 1] * sx;
        h.p[i + 2] = h.p[i + 2] * (h.H[i + 2] == h.H[i + 1] ? sx : std::sqrt(h.H[i + 2]));
      }
      T0[c] = kinetic(h.p.data(), h.H.data(), d, h.tmp);
      h.q0 = h.q;
      h.K0 = h.K;
      h.dead = false;
    });
    clock.lap(0);
    // 2. V(q)
    if (V_end.valid(R.mv.P)) {
      V0 = V_end.V;
    } else if (int rc = R.energies(all, V0)) {
      return rc;
    }
    parallel(pool, all, [&](int64_t c) {
      Chain& h = R.ch[c];
      h.E0 = V0[c] + T0[c];
      record_start(cfg, rec, l * rec_stride + rec_off + c, W, h.q.data(), h.p.data(), h.K, V0[c],
                   T0[c], h.E0, h.move, h.grow);
    });
    clock.lap(1);
    // 3. the trajectory of every chain
    if (int rc = R.trajectories(all)) return rc;
    clock.lap(2);
    // 4. the proposals
    std::vector<int64_t> jump;
    for (int64_t c = 0; c < n; ++c)
      if (R.ch[c].move != 0) jump.push_back(c);
    parallel(pool, jump, [&](int64_t c) {
      Chain& h = R.ch[c];
      for (auto& v : h.p) v = -v;
      if (!R.mv.propose(h, M)) {
        h.dead = true;
        h.q = h.q0;
        h.K = h.K0;
      }
    });
    std::vector<int64_t> live;
    for (int64_t c : jump)
      if (!R.ch[c].dead) live.push_back(c);
    clock.lap(3);
    // 5. the trajectory after the jump
    if (int rc = R.trajectories(live)) return rc;
    clock.lap(4);
    for (int64_t c : live)
      for (auto& v : R.ch[c].p) v = -v;
    // 6. V(q')
    std::vector<int64_t> scored;
    for (int64_t c = 0; c < n; ++c)
      if (!R.ch[c].dead) scored.push_back(c);
    if (int rc = R.energies(scored, V1)) return rc;
    clock.lap(5);
    // 7. accept / reject
    parallel(pool, all, [&](int64_t c) {
      Chain& h = R.ch[c];
      bool acc = false;
      if (!h.dead) {
        const int64_t d = 3 * (int64_t)h.K;
        h.H.resize((size_t)d);
        M.all(h.q.data(), d, h.H.data());
        const double E1 = V1[c] + kinetic(h.p.data(), h.H.data(), d, h.tmp);
        acc = accepts(h.move, h.E0, E1, std::log(h.rng.random_sample()), h.factor);
        if (!acc) {
          h.q = h.q0;
          h.K = h.K0;
        }
      }
      V_end.V[c] = acc ? V1[c] : V0[c];
      record_accept(rec, l * rec_stride + rec_off + c, acc, h.dead);
    });
    clock.lap(6);
    V_end.store(R.mv.P);
  }
  clock.add_to(phase_out);
  for (int64_t c = 0; c < n; ++c)
    finish_chain(R.ch[c], cfg, rec_off, c, R.ch[c].q.data(), W, W, q, K);
  return 0;
}

}  // namespace
