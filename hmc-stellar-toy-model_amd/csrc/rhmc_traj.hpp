// rhmc_traj.hpp — the random-length trajectory of samplers.lightsource_gym's
// HMC_random (samplers.py:519-552) and RHMC_random_diag (:766-800), once for
// every kernel family.  Included from rhmc_wave.hpp (DiagArgs, diag_force_f,
// diag_drift).
#pragma once

namespace rhmc {

// A lambda that the trajectory calls from more than one site: without the
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

}  // namespace rhmc
