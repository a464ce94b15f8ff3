// rj_moves.hpp — one chain's host state and the reversible-jump proposals
// (birth_death_move, split_merge_move) in the reference's operation order.
// A section of rhmc_rj.cpp's translation unit.
#pragma once

#include "rj_model.hpp"

namespace {

struct Chain {
  rhmc_np::Legacy rng;
  std::vector<double> q, p, q0;  // state, momentum, the iteration's starting q
  int32_t K = 0, K0 = 0;
  int move = 0;                  // 0 within, 1 birth/death, 2 split/merge
  bool grow = false, dead = false;
  double E0 = 0., factor = 0.;
  std::vector<double> H, tmp, cdf;
  // the device driver's draws made ahead, while the GPU runs: the accept
  // uniform, and the next iteration's normals / move / grow of a chain whose
  // star count cannot change (move 0 or a dead end) — the stream's order is
  // unchanged, only the time of the draws moves
  double u = 0.;
  bool pre = false, grow_next = false;
  int move_next = 0;
  std::vector<double> znext;
};

// What the moves read of a run: the engine parameters of the iteration (the
// schedules set P.g_ff2 / P.beta), the configuration, the star-count limit
// and the split fraction's density.
struct Moves {
  rhmc_params P;
  const rhmc_rj_config* cfg;
  int Kmax;
  BetaDist beta;

  Moves(const rhmc_params* P0, const rhmc_rj_config* c) : P(*P0), cfg(c), Kmax(c->N_max) {
    beta.set(c->beta_a, c->beta_b);
  }

  Metric metric() const {
    return Metric{P.g_ff2, P.g_ff, P.g_xx, P.g0, P.g1, P.g2, P.B_count, P.f_low};
  }

  // the proposal of chain c's move on (q, -p); false = dead end
  bool propose(Chain& c, const Metric& M) const {
    return c.move == 1 ? birth_death(c, M) : split_merge(c, M);
  }

  // birth_death_move (sampler_RHMC.py:1200-1270) on (q, -p); false = dead end
  bool birth_death(Chain& c, const Metric& M) const {
    const double alpha = P.alpha;
    if (c.grow) {
      if (c.K + 1 > Kmax) return false;
      const double x = c.rng.random_sample() * (cfg->rows - 2.) + 1.;    // :1219
      const double y = c.rng.random_sample() * (cfg->cols - 2.) + 1.;    // :1220
      const double u = c.rng.random_sample();                             // :1221
      const double e = 1 - alpha;                                         // utils.py:469-471
      const double lm = std::pow(cfg->fmin, e) + u * (std::pow(cfg->fmax, e) - std::pow(cfg->fmin, e));
      const double f = std::exp(std::log(lm) / e);
      const double qn[3] = {f, x, y};
      double H3[3], pn[3];
      M.star(f, H3);
      for (int i = 0; i < 3; ++i) pn[i] = c.rng.gauss() * std::sqrt(H3[i]);   // :1231
      c.factor = alpha * std::log(f) - 3 / 2. + kinetic(pn, H3, 3, c.tmp) + P.V_prior_const;
      c.q.insert(c.q.end(), qn, qn + 3);
      c.p.insert(c.p.end(), pn, pn + 3);
      c.K += 1;
    } else {
      if (c.K - 1 < 1) return false;
      const int64_t k = c.rng.randint(0, c.K);                            // :1249
      double H3[3];
      M.star(c.q[3 * k], H3);
      const double Tk = kinetic(&c.p[3 * k], H3, 3, c.tmp);
      c.factor = -alpha * std::log(c.q[3 * k]) + 3 / 2. - Tk - P.V_prior_const;
      c.q.erase(c.q.begin() + 3 * k, c.q.begin() + 3 * k + 3);
      c.p.erase(c.p.begin() + 3 * k, c.p.begin() + 3 * k + 3);
      c.K -= 1;
    }
    return true;
  }

  // split_merge_move (sampler_RHMC.py:1273-1445) on (q, -p); false = dead end
  bool split_merge(Chain& c, const Metric& M) const {
    const double a = cfg->beta_a, b = cfg->beta_b, Ks = cfg->K_split;
    const double two_pi_ks2 = 2 * kPi * std::pow(Ks, 2);
    const double ln_q_dxdy = std::log(two_pi_ks2);
    const double two_ks2 = 2 * std::pow(Ks, 2);
    if (c.grow) {
      if (c.K + 1 > Kmax) return false;
      const int64_t i = c.rng.randint(0, c.K);                            // :1291
      const double fs = c.q[3 * i], xs = c.q[3 * i + 1], ys = c.q[3 * i + 2];
      const double qs[3] = {fs, xs, ys}, ps[3] = {c.p[3 * i], c.p[3 * i + 1], c.p[3 * i + 2]};
      const double g1 = c.rng.gauss(), g2 = c.rng.gauss();                // :1300
      const double dx = g1 * Ks, dy = g2 * Ks;
      const double dr_sq = std::pow(dx, 2) + std::pow(dy, 2);
      const double F = c.rng.beta(a, b);                                  // :1302
      const double q1[3] = {F * fs, xs + (1 - F) * dx, ys + (1 - F) * dy};
      const double q2[3] = {(1 - F) * fs, xs - F * dx, ys - F * dy};
      double H1[3], H2[3], Hs[3], p1[3], p2[3];
      M.star(q1[0], H1);
      for (int t = 0; t < 3; ++t) p1[t] = c.rng.gauss() * std::sqrt(H1[t]);   // :1328
      M.star(q2[0], H2);
      for (int t = 0; t < 3; ++t) p2[t] = c.rng.gauss() * std::sqrt(H2[t]);   // :1333
      M.star(qs[0], Hs);
      const double Ts = kinetic(ps, Hs, 3, c.tmp);
      const double T1 = kinetic(p1, H1, 3, c.tmp), T2 = kinetic(p2, H2, 3, c.tmp);
      c.factor = (-3 / 2.) + std::log(fs) - beta.logpdf(F) + ln_q_dxdy + (dr_sq / two_ks2) +
                 T1 + T2 - Ts;
      for (int t = 0; t < 3; ++t) {
        c.q[3 * i + t] = q1[t];
        c.p[3 * i + t] = p1[t];
      }
      c.q.insert(c.q.end(), q2, q2 + 3);
      c.p.insert(c.p.end(), p2, p2 + 3);
      c.K += 1;
      return true;
    }
    const int64_t n = c.K;
    if (n - 1 < 1) return false;
    // pair probabilities ~ Beta(F_ij) N(r_ij), self pairs excluded (:1366-1378).
    // R_sq is symmetric bit for bit ((a - b)^2 == (b - a)^2), so each pair's
    // Gaussian factor is evaluated once for both orders
    std::vector<double> P2((size_t)(n * n));
    for (int64_t r = 0; r < n; ++r)
      for (int64_t s = r; s < n; ++s) {
        const double ddx = c.q[3 * r + 1] - c.q[3 * s + 1], ddy = c.q[3 * r + 2] - c.q[3 * s + 2];
        const double Rsq = std::pow(ddx, 2) + std::pow(ddy, 2);
        const double g = std::exp(-Rsq / two_ks2) / two_pi_ks2;
        const double fr = c.q[3 * r], fc = c.q[3 * s];
        const double F1 = fc / (fr + fc);
        double v1 = beta.pdf(F1);
        if (std::fabs(F1 - 0.5) < 1e-6) v1 = 0.;
        P2[r * n + s] = v1 * g;
        if (s == r) continue;
        const double F2 = fr / (fc + fr);
        double v2 = beta.pdf(F2);
        if (std::fabs(F2 - 0.5) < 1e-6) v2 = 0.;
        P2[s * n + r] = v2 * g;
      }
    const double tot = rhmc_np::pairwise_sum(P2.data(), n * n);
    if (!(tot > 0.0) || !std::isfinite(tot)) return false;  // the reference raises here
    for (auto& v : P2) v /= tot;
    const int64_t pair = choice(c.rng, P2.data(), n * n, c.cdf);          // :1381
    if (pair >= n * n) return false;
    const int64_t i1 = pair / n, i2 = pair % n;
    const double q1[3] = {c.q[3 * i1], c.q[3 * i1 + 1], c.q[3 * i1 + 2]};
    const double p1[3] = {c.p[3 * i1], c.p[3 * i1 + 1], c.p[3 * i1 + 2]};
    const double q2[3] = {c.q[3 * i2], c.q[3 * i2 + 1], c.q[3 * i2 + 2]};
    const double p2[3] = {c.p[3 * i2], c.p[3 * i2 + 1], c.p[3 * i2 + 2]};
    const double F = q1[0] / (q1[0] + q2[0]);
    const double dx = q1[1] - q2[1], dy = q1[2] - q2[2];
    const double dr_sq = std::pow(dx, 2) + std::pow(dy, 2);
    const double qs[3] = {q1[0] + q2[0], F * q1[1] + (1 - F) * q2[1], F * q1[2] + (1 - F) * q2[2]};
    double H1[3], H2[3], Hs[3], ps[3];
    M.star(q1[0], H1);
    const double T1 = kinetic(p1, H1, 3, c.tmp);
    M.star(q2[0], H2);
    const double T2 = kinetic(p2, H2, 3, c.tmp);
    M.star(qs[0], Hs);
    for (int t = 0; t < 3; ++t) ps[t] = c.rng.gauss() * std::sqrt(Hs[t]);      // :1415
    const double Ts = kinetic(ps, Hs, 3, c.tmp);
    const int64_t lo = std::min(i1, i2), hi = std::max(i1, i2);
    std::vector<double> nq, np_;
    nq.reserve((size_t)(3 * (n - 1)));
    np_.reserve((size_t)(3 * (n - 1)));
    for (int64_t s = 0; s < n; ++s) {
      if (s == lo || s == hi) continue;
      nq.insert(nq.end(), &c.q[3 * s], &c.q[3 * s] + 3);
      np_.insert(np_.end(), &c.p[3 * s], &c.p[3 * s] + 3);
    }
    nq.insert(nq.end(), qs, qs + 3);
    np_.insert(np_.end(), ps, ps + 3);
    c.factor = (3 / 2.) - std::log(qs[0]) + beta.logpdf(F) - ln_q_dxdy - (dr_sq / two_ks2) -
               T1 - T2 + Ts;
    c.q.swap(nq);
    c.p.swap(np_);
    c.K -= 1;
    return true;
  }
};

}  // namespace
