// rhmc_traj.hpp — the random-length trajectory of samplers.lightsource_gym's
// HMC_random (samplers.py:519-552) and RHMC_random_diag (:766-800), once for
// every kernel family (random_trajectory), RHMC_random's (:1016-1067,
// hess_trajectory), and single_gym's explicit integrators, once for every
// kernel family (explicit_steps).  Included from rhmc_wave.hpp (DiagArgs,
// diag_force_f, diag_drift).
#pragma once

#include "rhmc.h"

namespace rhmc {

// A lambda that a shared loop calls from more than one site: without the
// attribute a gradient wrapped in one is not inlined at 8 slots and its array
// arguments go to scratch.
#define RHMC_INLINE_LAMBDA __attribute__((always_inline))

// HMC_random's trajectory for SLOTS stars per lane: unit-mass leapfrog of n
// steps with a step per star and coordinate, the flux wall at f_lim.  The
// reference's quirks are kept: a star's flip flag `iflip` is never cleared
// within a trajectory, and the flip applies on every step in which ANY star
// of the chain is below the wall, so a star once below it has its flux
// momentum flipped on every such later step (:526-541); and when the last step
// flipped, p_tmp keeps the momentum the trajectory started from (:547-550
// update p_half, not p_tmp).  So: p holds the start momentum on entry, the
// half-step momentum during the steps and the end momentum on return; the
// return value says that the last step flipped, and the caller then puts the
// start momentum back and sets RHMC_STATUS_REFLECT_F.  dVdq is without the
// metric (:365-425).
// DIAG: RHMC_random_diag's trajectory instead: the one step dg.dt, the drift
// divided by the mass matrix at the flux before it (diag_drift), dlnDetdq +
// dpMpdq in the flux force (diag_force_f) from the START momentum's squares on
// every step, the same wall quirks, and q after every step to the trace.
//
// What a family does its own way comes in as callables:
//   step(t, j)            the step of slot t, coordinate j (HMC_random only)
//   own(t)                the lane has a star in slot t
//   any(b)                b of any lane of the chain
//   grad(gf, gx, gy)      dVdq with the prior at the current f, x, y, with
//                         whatever the family does around it (star table)
//   start_sq(t, sf, sxy)  DIAG: pf^2 and px^2 + py^2 of the start momentum
//   trace(row)            DIAG: q to row `row` of the chain's trace
template <int SLOTS, bool DIAG, class STEP, class OWN, class ANY, class GRAD, class SSQ,
          class TRACE>
__device__ __forceinline__ bool random_trajectory(double (&f)[SLOTS], double (&x)[SLOTS],
                                                  double (&y)[SLOTS], double (&pf)[SLOTS],
                                                  double (&px)[SLOTS], double (&py)[SLOTS], int n,
                                                  double f_lim, const DiagArgs& dg, STEP step,
                                                  OWN own, ANY any, GRAD grad, SSQ start_sq,
                                                  TRACE trace) {
  auto dt = [&](int t, int j) RHMC_INLINE_LAMBDA {
    if constexpr (DIAG) return dg.dt;
    else return step(t, j);
  };
  double gf[SLOTS], gx[SLOTS], gy[SLOTS];
  auto force = [&]() RHMC_INLINE_LAMBDA {
    grad(gf, gx, gy);
    if constexpr (DIAG) {                          // dVdq + dlnDetdq + dpMpdq (:766)
#pragma unroll
      for (int t = 0; t < SLOTS; ++t) {
        double sf, sxy;
        start_sq(t, sf, sxy);
        gf[t] = diag_force_f(gf[t], f[t], sf, sxy, dg.inv_f1);
      }
    }
  };
  if constexpr (DIAG) trace(0);
  force();
  bool iflip[SLOTS];
#pragma unroll
  for (int t = 0; t < SLOTS; ++t) {                // :519
    pf[t] = pf[t] - dt(t, 0) * gf[t] / 2.0;
    px[t] = px[t] - dt(t, 1) * gx[t] / 2.0;
    py[t] = py[t] - dt(t, 2) * gy[t] / 2.0;
    iflip[t] = false;
  }
  bool flip = false;
  for (int s = 0; s < n; ++s) {
    bool below_any = false;
#pragma unroll
    for (int t = 0; t < SLOTS; ++t) {
      if constexpr (DIAG) {                        // :770-771
        diag_drift(f[t], x[t], y[t], pf[t], px[t], py[t], dg.dt, dg.inv_f1);
      } else {
        f[t] = f[t] + dt(t, 0) * pf[t];            // :523
        x[t] = x[t] + dt(t, 1) * px[t];
        y[t] = y[t] + dt(t, 2) * py[t];
      }
      const bool below = own(t) && f[t] < f_lim;   // :526-529
      if (below) iflip[t] = true;
      below_any = below_any || below;
    }
    flip = any(below_any);
    if constexpr (DIAG) trace(s + 1);
    force();
#pragma unroll
    for (int t = 0; t < SLOTS; ++t) {
      const double kept = -pf[t];                  // :531
      pf[t] = pf[t] - dt(t, 0) * gf[t];            // :532, :535
      px[t] = px[t] - dt(t, 1) * gx[t];
      py[t] = py[t] - dt(t, 2) * gy[t];
      if (flip && iflip[t]) pf[t] = kept;          // :533
    }
  }
  if (!flip) {                                     // :551-552, dVdq at the same q as the last step
#pragma unroll
    for (int t = 0; t < SLOTS; ++t) {
      pf[t] = pf[t] + dt(t, 0) * gf[t] / 2.0;
      px[t] = px[t] + dt(t, 1) * gx[t] / 2.0;
      py[t] = py[t] + dt(t, 2) * gy[t] / 2.0;
    }
  }
  return flip;
}

// n_steps steps of single_gym's explicit integrators for SLOTS stars per lane,
// once for every kernel family: plain HMC, unit metric (sampler_RHMC.py
// :628-645), explicit RHMC "naive" (:690-708) and "leap_frog" (:709-728), the
// flux wall at f_lim under f_pos.  The gradient at the end of a step is the
// next step's first one (same q).  A flip takes the momentum from before the
// kick, and only a lane that owns the star sets RHMC_STATUS_REFLECT_F.
// What a family does its own way comes in as callables:
//   force(gf, gx, gy)  dVdq (:365-425) at the current f, x, y with the flux
//                      prior where the family adds it, with whatever the family
//                      does around the gradient, and the family's metric at
//                      that state where metric(t) reads it
//   metric(t)          slot t's metric at the state of the last force(), as a
//                      view: over_Hff(v) = v / H_ff, over_Hxx(v) = v / H_xx and
//                      force_f(p), dVdq_RHMC's flux slot (:427-446; its position
//                      slots are 0).  Not called for HMC.
//   own(t)             the lane has a star in slot t
//   moved()            after every update of q
template <int SOLVER, int SLOTS, class FORCE, class METRIC, class OWN, class MOVED>
__device__ __forceinline__ void explicit_steps(double (&f)[SLOTS], double (&x)[SLOTS],
                                               double (&y)[SLOTS], double (&pf)[SLOTS],
                                               double (&px)[SLOTS], double (&py)[SLOTS],
                                               int n_steps, int f_pos, double f_lim, double dt,
                                               unsigned& st, FORCE force, METRIC metric, OWN own,
                                               MOVED moved) {
  double gf[SLOTS], gx[SLOTS], gy[SLOTS];
  if constexpr (SOLVER == RHMC_SOLVER_RHMC_NAIVE) {
    // the gradient opens each step (nothing of it lives across steps)
    for (int s = 0; s < n_steps; ++s) {
      force(gf, gx, gy);
#pragma unroll
      for (int t = 0; t < SLOTS; ++t) {
        const auto m = metric(t);
        const double nf = f[t] + m.over_Hff(dt * pf[t]);       // :692
        x[t] = x[t] + m.over_Hxx(dt * px[t]);
        y[t] = y[t] + m.over_Hxx(dt * py[t]);
        const double pf_old = pf[t];
        pf[t] = pf[t] - dt * (gf[t] + m.force_f(pf[t]));       // :696
        px[t] = px[t] - dt * gx[t];
        py[t] = py[t] - dt * gy[t];
        if (f_pos && nf < f_lim) {                             // :698-704, the new flux
          pf[t] = pf_old * -1.0;
          if (own(t)) st |= RHMC_STATUS_REFLECT_F;
        }
        f[t] = nf;
      }
      moved();
    }
  } else {
    // One gradient call site (the gradient is most of a kernel): pass s closes
    // step s - 1 and opens step s; p holds the half-step momentum across the
    // gradient.
    for (int s = 0;; ++s) {
      force(gf, gx, gy);
      if (s > 0) {                                             // second half kick of step s - 1
#pragma unroll
        for (int t = 0; t < SLOTS; ++t) {
          if constexpr (SOLVER == RHMC_SOLVER_HMC) {           // :638
            pf[t] = pf[t] - dt * gf[t] / 2.0;
          } else {                                             // :717-725
            const double hf = pf[t];
            pf[t] = hf - dt * (gf[t] + metric(t).force_f(hf)) / 2.0;
            if (f_pos && f[t] < f_lim) {                       // the flux of this gradient
              pf[t] = hf * -1.0;
              if (own(t)) st |= RHMC_STATUS_REFLECT_F;
            }
          }
          px[t] = px[t] - dt * gx[t] / 2.0;
          py[t] = py[t] - dt * gy[t] / 2.0;
        }
      }
      if (s == n_steps) break;
#pragma unroll
      for (int t = 0; t < SLOTS; ++t) {                        // first half kick and drift of step s
        if constexpr (SOLVER == RHMC_SOLVER_HMC) {             // :631-634
          pf[t] = pf[t] - dt * gf[t] / 2.0;
          px[t] = px[t] - dt * gx[t] / 2.0;
          py[t] = py[t] - dt * gy[t] / 2.0;
          f[t] = f[t] + dt * pf[t];
          x[t] = x[t] + dt * px[t];
          y[t] = y[t] + dt * py[t];
        } else {                                               // :711-714
          const auto m = metric(t);
          pf[t] = pf[t] - dt * (gf[t] + m.force_f(pf[t])) / 2.0;
          px[t] = px[t] - dt * gx[t] / 2.0;
          py[t] = py[t] - dt * gy[t] / 2.0;
          f[t] = f[t] + m.over_Hff(dt * pf[t]);
          x[t] = x[t] + m.over_Hxx(dt * px[t]);
          y[t] = y[t] + m.over_Hxx(dt * py[t]);
        }
      }
      moved();
    }
  }
}

// One star's derivative sets of RHMC_efficient_computation (samplers.py:881-903):
// dVdq, dVdqq and dVdqqq for (f, x, y).
struct HessD {
  double d1f, d1x, d1y, d2f, d2x, d2y, d3f, d3x, d3y;
};

// RHMC_random's trajectory (samplers.py:1016-1067) for one star per lane:
// leapfrog under the metric diag(dVdqq), the force with dVdqqq, steps dt_f for
// f and dt_xy for x and y.  On entry (f, x, y) and (pf, px, py) are the start;
// on return q is the end state, p the reference's p_half, D the derivative
// sets at the end q; the return value is the number of completed steps.
// The reference's quirks, all kept:
//   * dVdqq is used as it comes, negative or zero included: nothing guards the
//     divisions, NaN and inf propagate (:909-911);
//   * below the wall RHMC_efficient_computation returns three scalar infs
//     (:836-837), so every coordinate's dpdt is +inf there: a chain that starts
//     below it gets p + dt inf / 2 (:1016) and does no step, and after a
//     crossing in mid-trajectory p_half += dt' inf (:1058) leaves +-inf, or NaN
//     where dt' is 0, in every entry that is not flagged;
//   * a step begins with the test E(q, p_half) == +inf (:1024-1027) and breaks
//     on it.  V is finite or NaN while f_lim >= 0, so the test holds iff some
//     f < f_lim, or K (:911) is +inf and every coordinate of q is finite: no
//     logarithm per pixel, one per chain and step (the callers refuse
//     f_lim < 0);
//   * the two calls of a step (:1024, :1054) and the first call of the next
//     step differ only in p: derivs() runs once per step;
//   * the flux flag is sticky per star and applied on every step in which ANY
//     star of the chain is below the wall (:1035-1037, :1060-1061);
//   * the position flags test (x < 0) or (x < num_rows), y against num_rows
//     too (:1038-1043): true for every coordinate below the side, so px and py
//     of a star inside the image are replaced by their negatives on every step
//     and never receive the force; a star at x >= num_rows or NaN does not set
//     the switch but, once flagged, is still flipped when another star sets it
//     (:1063-1067);
//   * the last step adds dt / 2 (:1046-1047) and there is no closing un-kick;
//     the flagged entries take -p_half from before the update (:1057).
// What the kernel does its own way comes in as callables:
//   own()       the lane has a star
//   any(b)      b of any lane of the chain
//   sum(v)      v summed over the chain's lanes
//   prod()      dVdqq's running product over the chain in index order (:911)
//   derivs(D)   D at the current (f, x, y)
template <class OWN, class ANY, class SUM, class PROD, class DERIVS>
__device__ __forceinline__ int hess_trajectory(double& f, double& x, double& y, double& pf,
                                               double& px, double& py, int n, double f_lim,
                                               double side, double dt_f, double dt_xy, HessD& D,
                                               bool& flag_f, bool& flag_xy, OWN own, ANY any,
                                               SUM sum, PROD prod, DERIVS derivs) {
  const double inf = __builtin_inf();
  const bool me = own();
  auto dpdt = [&](bool wall, double p, double d1, double d2, double d3) RHMC_INLINE_LAMBDA {
    const double dqdt = p / d2;                                      // :909
    const double v = -d3 * ((1. / d2) - dqdt * dqdt) / 2. - d1;      // :910
    return wall ? inf : v;
  };
  derivs(D);
  bool wall = any(me && f < f_lim);                // :832-837
  pf = pf + dt_f * dpdt(wall, pf, D.d1f, D.d2f, D.d3f) / 2.;   // :1016
  px = px + dt_xy * dpdt(wall, px, D.d1x, D.d2x, D.d3x) / 2.;
  py = py + dt_xy * dpdt(wall, py, D.d1y, D.d2y, D.d3y) / 2.;
  bool iflip = false, iflip_x = false, iflip_y = false;
  int done = 0;
  for (int z = 0; z < n; ++z) {
    const double kin =
        sum(me ? (pf * pf) / D.d2f + (px * px) / D.d2x + (py * py) / D.d2y : 0.0);
    const double K = kin / 2. + log(prod()) / 2.;                    // :911
    const bool q_finite = !any(me && !(isfinite(f) && isfinite(x) && isfinite(y)));
    if (wall || (K == inf && q_finite)) break;                       // :1025-1027
    f = f + dt_f * (pf / D.d2f);                                     // :1031
    x = x + dt_xy * (px / D.d2x);
    y = y + dt_xy * (py / D.d2y);
    const bool below = me && f < f_lim;                              // :1035
    const bool in_x = me && (x < 0.0 || x < side);                   // :1038
    const bool in_y = me && (y < 0.0 || y < side);                   // :1041
    iflip = iflip || below;
    iflip_x = iflip_x || in_x;
    iflip_y = iflip_y || in_y;
    const bool flip = any(below), flip_x = any(in_x), flip_y = any(in_y);
    wall = flip;
    derivs(D);                                                       // :1054
    const bool last = z == n - 1;                                    // :1046-1049
    const double tf = last ? dt_f / 2. : dt_f, txy = last ? dt_xy / 2. : dt_xy;
    const double kf = -pf, kx = -px, ky = -py;                       // :1057
    pf = pf + tf * dpdt(wall, pf, D.d1f, D.d2f, D.d3f);              // :1058
    px = px + txy * dpdt(wall, px, D.d1x, D.d2x, D.d3x);
    py = py + txy * dpdt(wall, py, D.d1y, D.d2y, D.d3y);
    if (flip && iflip) pf = kf;                                      // :1060-1067
    if (flip_x && iflip_x) px = kx;
    if (flip_y && iflip_y) py = ky;
    ++done;
  }
  flag_f = iflip;
  flag_xy = iflip_x || iflip_y;
  return done;
}

}  // namespace rhmc
