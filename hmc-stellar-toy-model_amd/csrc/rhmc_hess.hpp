// rhmc_hess.hpp — the kernels of samplers.lightsource_gym.RHMC_random
// (samplers.py:828-1105), the sampler whose metric is the diagonal of the
// likelihood's Hessian: hess_derivs_kernel (q -> dVdq, dVdqq, dVdqqq, V) and
// hess_random_kernel (the trajectory, hess_trajectory of rhmc_traj.hpp).
// Device code only; select_hess() (rhmc_select.hpp) sizes the workgroup and
// launch_hess() (rhmc_launch.hpp) launches them.
//
// Work decomposition: one wave64 per chain, lane k < K holds star k for the
// whole trajectory; a workgroup of W waves shares the fp64 image, staged once
// into LDS.  Served: 1 <= K <= 16, square images of side 16..48 (side <= 64
// lanes is what the second pass needs).
//
// One derivative set costs one pass over the image plus one pass per star:
//   * pass 1, lanes over pixels: Lambda = B + sum_k f_k ex_k[i] ey_k[j] from
//     the separable factor tables of rhmc_perwave.hpp (build_tables), and
//     s = 1 / Lambda into the wave's own LDS image.  With D in LDS the three
//     weights are products: r0 = D s, r1 = 1 - r0, r2 = r0 s, r3 = r2 s.
//   * pass 2, per star, lane l = row l and column l: every derivative of the
//     PSF is the PSF times a polynomial in the row offset alone or the column
//     offset alone, so the fifteen sums of samplers.py:881-893 follow from six
//     separable accumulations,
//       R_m[i] = sum_j ey[j]^m r_m[i][j],  C_m[j] = sum_i ex[i]^m r_m[i][j],
//     m = 1, 2, 3; lane l then weighs R_m[l] with ex[l]^m and the polynomial
//     in dx[l] = (l + .5) - x, C_m[l] likewise, and nine butterfly sums give
//     the star's dVdq, dVdqq, dVdqqq.  Lane l walks its row from column l on
//     (stride side + 1 doubles across lanes: no bank conflict of the row-major
//     image) and its column from row 0.
// Per-star accumulators for 16 stars x 15 sums do not fit in registers, hence
// the star loop outside the pixels.  The arithmetic is contracted nowhere but
// in the fma() calls written out, so both kernels give the same bits at the
// same q.
#pragma once
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>

#include "rhmc.h"
#include "rhmc_perwave.hpp"
#include "rhmc_select.hpp"
#include "rhmc_traj.hpp"
#include "rhmc_wave.hpp"

namespace rhmc {

struct HessArgs {
  double* q;               // [n][3K]; hess_derivs_kernel only reads it
  double* p;               // [n][3K] (trajectory)
  const int32_t* steps;    // [n]     (trajectory)
  int32_t* status;         // nullable
  int32_t* steps_done;     // nullable
  double* dVdq;            // nullable [n][3K]
  double* dVdqq;
  double* dVdqqq;
  double* V;               // nullable [n] (hess_derivs_kernel)
  const double* D;
  int64_t n_chains;
  int K;
  double dt_f, dt_xy;
  Geometry g;
  Consts c;
};

// A wave's LDS after the shared image: tables, the 1 / Lambda image, fluxes.
struct HessLds {
  Tables tab;
  double* inv;   // [side][side]
  double* fk;    // [kMaxKGeneric]
};

__device__ __forceinline__ HessLds hess_carve(double* lds, int K, const Geometry& g) {
  double* base = lds + g.npix + (threadIdx.x / kWave) * hess_wave_doubles(K, g.rows);
  HessLds h;
  h.tab = carve_tables(base, K, g);
  h.inv = base + table_doubles(K, g.rows, g.cols);
  h.fk = h.inv + g.npix;
  return h;
}

// The derivative sets of the chain of this wave at (f, x, y): lane k < K gets
// star k's in D (other lanes keep theirs); V = -sum(D ln Lambda - Lambda) with
// WITH_V (every lane), else untouched.
template <bool WITH_V>
__device__ __forceinline__ void hess_derivs(const double* __restrict__ sD, const HessLds& h,
                                            int K, double f, double x, double y,
                                            const Geometry& g, const Consts& c, HessD& D,
                                            double& V) {
#pragma clang fp contract(off)
  const int lane = lane_id();
  const int side = g.rows;
  const Tables& t = h.tab;
  if (lane < K) h.fk[lane] = f;
  build_tables(t, K, x, y, g, c);  // ends with the wave's LDS hand-off

  // pass 1: Lambda (:845-848) and its reciprocal
  double v = 0.0;
  {
    int i = lane / side, j = lane - (lane / side) * side;
    for (int pix = lane; pix < g.npix; pix += kWave) {
      double lam = c.B;
      for (int k = 0; k < K; ++k)
        lam = fma(h.fk[k], t.ex[k * side + i] * t.ey[k * side + j], lam);
      h.inv[pix] = 1.0 / lam;
      if constexpr (WITH_V) v += sD[pix] * log(lam) - lam;           // :912
      j += g.dj;
      i += g.di;
      if (j >= side) {
        j -= side;
        ++i;
      }
    }
  }
  if constexpr (WITH_V) V = -wave_sum(v);
  wave_lds_sync();

  // pass 2: per star the six separable accumulations, then the weights
  const bool active = lane < side;
  const int l = active ? lane : 0;
  for (int k = 0; k < K; ++k) {
    const double* ex = t.ex + k * side;
    const double* ey = t.ey + k * side;
    double r1 = 0.0, r2 = 0.0, r3 = 0.0, c1 = 0.0, c2 = 0.0, c3 = 0.0;
    if (active) {
      int jj = l;
      for (int tt = 0; tt < side; ++tt) {
        {  // row l, column jj
          const double s = h.inv[l * side + jj];
          const double rho0 = sD[l * side + jj] * s;                 // :851-854
          const double rho1 = 1.0 - rho0, rho2 = rho0 * s;
          const double rho3 = rho2 * s;
          const double e = ey[jj], e2 = e * e;
          r1 = fma(e, rho1, r1);
          r2 = fma(e2, rho2, r2);
          r3 = fma(e2 * e, rho3, r3);
        }
        {  // column l, row tt
          const double s = h.inv[tt * side + l];
          const double rho0 = sD[tt * side + l] * s;
          const double rho1 = 1.0 - rho0, rho2 = rho0 * s;
          const double rho3 = rho2 * s;
          const double e = ex[tt], e2 = e * e;
          c1 = fma(e, rho1, c1);
          c2 = fma(e2, rho2, c2);
          c3 = fma(e2 * e, rho3, c3);
        }
        jj = jj + 1 == side ? 0 : jj + 1;
      }
    }
    const double fs = h.fk[k], fs2 = fs * fs;
    const double fs3 = fs2 * fs;
    double w[9];
    {  // rows: P = ex ey, P_x = P a, P_xx = P b, P_xxx = P d (:869-872)
      const double e = active ? ex[l] : 0.0, dx = t.dx[k * side + l];
      const double a = dx / c.var;
      const double b = (a * dx - 1.0) / c.var;
      const double d = (b * dx - 2.0 * a) / c.var;
      const double S1 = e * r1, S2 = (e * e) * r2, S3 = (e * e * e) * r3;
      w[0] = S1;                                                     // :881-883
      w[3] = S2;
      w[6] = -2.0 * S3;
      w[1] = fs * (a * S1);                                          // :885-888
      w[4] = fs2 * ((a * a) * S2) + fs * (b * S1);
      w[7] = -fs3 * ((a * a * a) * S3) + 3.0 * fs2 * ((a * b) * S2) + fs * (d * S1);
    }
    {  // columns (:874-877, :890-893)
      const double e = active ? ey[l] : 0.0, dy = t.dy[k * side + l];
      const double a = dy / c.var;
      const double b = (a * dy - 1.0) / c.var;
      const double d = (b * dy - 2.0 * a) / c.var;
      const double T1 = e * c1, T2 = (e * e) * c2, T3 = (e * e * e) * c3;
      w[2] = fs * (a * T1);
      w[5] = fs2 * ((a * a) * T2) + fs * (b * T1);
      w[8] = -fs3 * ((a * a * a) * T3) + 3.0 * fs2 * ((a * b) * T2) + fs * (d * T1);
    }
#pragma unroll
    for (int m = 0; m < 9; ++m) w[m] = wave_sum(w[m]);
    if (lane == k) D = HessD{w[0], w[1], w[2], w[3], w[4], w[5], w[6], w[7], w[8]};
  }
  // the tables and the image are rewritten by the next call
  wave_lds_sync();
}

// Lane k < K's star of chain `chain`; the other lanes mirror star 0.
__device__ __forceinline__ int64_t hess_base(int64_t chain, int K, bool owner) {
  return chain * 3 * (int64_t)K + 3 * (owner ? lane_id() : 0);
}

__device__ __forceinline__ void hess_store_derivs(const HessArgs& a, int64_t base, bool owner,
                                                  const HessD& D) {
  if (!owner) return;
  if (a.dVdq) {
    a.dVdq[base] = D.d1f;
    a.dVdq[base + 1] = D.d1x;
    a.dVdq[base + 2] = D.d1y;
  }
  if (a.dVdqq) {
    a.dVdqq[base] = D.d2f;
    a.dVdqq[base + 1] = D.d2x;
    a.dVdqq[base + 2] = D.d2y;
  }
  if (a.dVdqqq) {
    a.dVdqqq[base] = D.d3f;
    a.dVdqqq[base + 1] = D.d3x;
    a.dVdqqq[base + 2] = D.d3y;
  }
}

// q -> dVdq, dVdqq, dVdqqq [n][3K] and V [n] (each nullable); no wall check,
// like RHMC_efficient_computation(dVdqq_only=True).
__global__ void __launch_bounds__(256) hess_derivs_kernel(HessArgs a) {
  extern __shared__ double lds[];
  const Geometry& g = a.g;
  const int64_t chain = stage_image(lds, a.D, g.npix, blockDim.x / kWave);
  if (chain >= a.n_chains) return;
  const int K = a.K;
  const HessLds h = hess_carve(lds, K, g);
  const bool owner = lane_id() < K;
  const int64_t base = hess_base(chain, K, owner);
  const double f = a.q[base], x = a.q[base + 1], y = a.q[base + 2];
  HessD D{1., 1., 1., 1., 1., 1., 1., 1., 1.};
  double V = 0.0;
  if (a.V) hess_derivs<true>(lds, h, K, f, x, y, g, a.c, D, V);
  else hess_derivs<false>(lds, h, K, f, x, y, g, a.c, D, V);
  hess_store_derivs(a, base, owner, D);
  if (a.V && lane_id() == 0) a.V[chain] = V;
}

// The trajectory of steps[chain] steps from (q, p), in place; status,
// steps_done and the derivative sets at the end state are nullable.
__global__ void __launch_bounds__(256) hess_random_kernel(HessArgs a) {
  extern __shared__ double lds[];
  const Geometry& g = a.g;
  const Consts& c = a.c;
  const int64_t chain = stage_image(lds, a.D, g.npix, blockDim.x / kWave);
  if (chain >= a.n_chains) return;
  const int K = a.K;
  const HessLds h = hess_carve(lds, K, g);
  const bool owner = lane_id() < K;
  const int64_t base = hess_base(chain, K, owner);
  double f = a.q[base], x = a.q[base + 1], y = a.q[base + 2];
  double pf = a.p[base], px = a.p[base + 1], py = a.p[base + 2];
  HessD D{1., 1., 1., 1., 1., 1., 1., 1., 1.};
  bool flag_f = false, flag_xy = false;
  const int done = hess_trajectory(
      f, x, y, pf, px, py, a.steps[chain], c.f_lim, (double)g.rows, a.dt_f, a.dt_xy, D, flag_f,
      flag_xy, [&]() RHMC_INLINE_LAMBDA { return owner; },
      [&](bool b) RHMC_INLINE_LAMBDA { return __any(b) != 0; },
      [&](double v) RHMC_INLINE_LAMBDA { return wave_sum(v); },
      [&]() RHMC_INLINE_LAMBDA {
        double pr = 1.0;
        for (int k = 0; k < K; ++k) {
          pr = pr * bcast(D.d2f, k);
          pr = pr * bcast(D.d2x, k);
          pr = pr * bcast(D.d2y, k);
        }
        return pr;
      },
      [&](HessD& o) RHMC_INLINE_LAMBDA {
        double V;
        hess_derivs<false>(lds, h, K, f, x, y, g, c, o, V);
      });
  unsigned st = 0u;
  if (owner) {
    if (flag_f) st |= RHMC_STATUS_REFLECT_F;
    if (flag_xy) st |= RHMC_STATUS_REFLECT_XY;
    if (!(isfinite(f) && isfinite(x) && isfinite(y) && isfinite(pf) && isfinite(px) &&
          isfinite(py)))
      st |= RHMC_STATUS_NONFINITE;
    a.q[base] = f;
    a.q[base + 1] = x;
    a.q[base + 2] = y;
    a.p[base] = pf;
    a.p[base + 1] = px;
    a.p[base + 2] = py;
  }
  hess_store_derivs(a, base, owner, D);
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) st |= (unsigned)__shfl_xor((int)st, m, kWave);
  if (lane_id() == 0) {
    if (a.status) a.status[chain] = (int32_t)st;
    if (a.steps_done) a.steps_done[chain] = done;
  }
}

}  // namespace rhmc
