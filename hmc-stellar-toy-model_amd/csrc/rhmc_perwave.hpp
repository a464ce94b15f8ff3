// rhmc_perwave.hpp — the one-wave-per-chain kernels of the RHMC leapfrog
// engine: the slotted *_win_kernel templates, which run a gradient policy (LdsG
// below, WinG / WinEG / WinGG of rhmc_windowed.hpp, DenseG of rhmc_dense.hpp),
// and the LDS-image step leapfrog_kernel<MAXK>.  The energy's T, support test,
// prior and pair potential and the gradient's frame are written once in the
// slotted kernels; a policy is where the image and the tables live, and the
// pixel loop.  The LDS-image step (K <= 16) keeps its own kernel: run through
// the slotted frame it lost 8 % at MAXK = 16.  Device
// code only: the host side that selects and launches them is rhmc_select.hpp /
// rhmc_launch.hpp.
//
// Work decomposition: one wave64 per chain, n_steps steps fused in one launch
// with (q, p) in registers.  LDS-image (LdsG, leapfrog_kernel): a workgroup of
// W waves shares the data image D, staged once into LDS with coalesced loads;
// after that single workgroup barrier every wave runs its chain independently
// (only wave-local LDS hand-offs).
//
// Per LDS-image gradient evaluation (the inner loop, sampler_RHMC.py:365-425):
//   * the Gaussian PSF is separable: PSF[i][j] = ex[i]*ey[j] with
//     ex[i] = exp(-((i+.5)-x)^2/(2s^2)), ey[j] = exp(-((j+.5)-y)^2/(2s^2))/(2 pi s^2)
//     -> (R + C) exps per star instead of R*C (utils.py:475-486);
//   * the per-wave LDS tables hold ex, ey and the offsets (i-x)+.5, (j-y)+.5;
//   * lane l owns pixels l, l+64, ...: Lambda = B + sum_k f_k psf_k,
//     w_k = psf_k*(D/Lambda - 1), three running sums per star;
//   * one butterfly all-reduce per sum.
// The end-of-step gradient (sampler_RHMC.py:551) is evaluated at the same q
// as the next step's first one (:525) — reflection only flips p — so it is
// carried over: one gradient per step, bit-identical to recomputing it.
#pragma once
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>

#include "rhmc.h"
#include "rhmc_select.hpp"
#include "rhmc_wave.hpp"
#include "rhmc_windowed.hpp"

namespace rhmc {

struct Tables {  // per-wave LDS tables, K stars
  double* ex;  // [K][rows]
  double* dx;  // [K][rows]
  double* ey;  // [K][cols]  (carries 1/(2 pi s^2))
  double* dy;  // [K][cols]
};

__device__ __forceinline__ Tables carve_tables(double* base, int K, const Geometry& g) {
  Tables t;
  t.ex = base;
  t.dx = base + K * g.rows;
  t.ey = base + 2 * K * g.rows;
  t.dy = base + 2 * K * g.rows + K * g.cols;
  return t;
}

// Build the separable PSF tables of K stars (lane k < K holds star k).
__device__ __forceinline__ void build_tables(const Tables& t, int K, double x, double y,
                                             const Geometry& g, const Consts& c) {
  const int lane = lane_id();
  const int span = g.rows + g.cols;
  for (int k = 0; k < K; ++k) {
    const double xk = bcast(x, k), yk = bcast(y, k);
    for (int e = lane; e < span; e += kWave) {
      if (e < g.rows) {
        const double v = (e + 0.5) - xk;
        t.ex[k * g.rows + e] = exp(-(v * v) / c.two_sig2);
        t.dx[k * g.rows + e] = ((double)e - xk) + 0.5;
      } else {
        const int j = e - g.rows;
        const double v = (j + 0.5) - yk;
        t.ey[k * g.cols + j] = exp(-(v * v) / c.two_sig2) / c.psf_norm;
        t.dy[k * g.cols + j] = ((double)j - yk) + 0.5;
      }
    }
  }
  wave_lds_sync();
}

// dVdq (optionally + the dphidq metric term) for the chain of this wave.
// Returns lane k's (g_f, g_x, g_y) for k < K; other lanes get junk.
template <int MAXK>
__device__ void gradient(const double* __restrict__ sD, const Tables& t, int K, double f,
                         double x, double y, const Geometry& g, const Consts& c,
                         bool with_metric, double& gf, double& gx, double& gy) {
  const int lane = lane_id();
  build_tables(t, K, x, y, g, c);

  double fk[MAXK];
#pragma unroll
  for (int k = 0; k < MAXK; ++k) fk[k] = (k < K) ? bcast(f, k) : 0.0;

  double acc[MAXK][3];
#pragma unroll
  for (int k = 0; k < MAXK; ++k) acc[k][0] = acc[k][1] = acc[k][2] = 0.0;

  int i = lane / g.cols, j = lane - (lane / g.cols) * g.cols;
  for (int tt = 0; tt < g.npl; ++tt) {
    const int pix = lane + kWave * tt;
    if (pix < g.npix) {
      const double dv = sD[pix];
      double psf[MAXK];
      double lam = c.B;  // Lambda = B + sum_k f_k PSF_k (:373-376)
#pragma unroll
      for (int k = 0; k < MAXK; ++k) {
        if (k < K) {
          psf[k] = t.ex[k * g.rows + i] * t.ey[k * g.cols + j];
          lam = fma(fk[k], psf[k], lam);
        }
      }
      const double r = dv / lam;  // rho + 1 = D/Lambda (:379)
#pragma unroll
      for (int k = 0; k < MAXK; ++k) {
        if (k < K) {
          const double w = fma(psf[k], r, -psf[k]);  // rho * PSF
          acc[k][0] += w;
          acc[k][1] = fma(w, t.dx[k * g.rows + i], acc[k][1]);
          acc[k][2] = fma(w, t.dy[k * g.cols + j], acc[k][2]);
        }
      }
    }
    j += g.dj;
    i += g.di;
    if (j >= g.cols) {
      j -= g.cols;
      ++i;
    }
  }

  gf = gx = gy = 0.0;
#pragma unroll
  for (int k = 0; k < MAXK; ++k) {
    if (k < K) {
      const double s0 = wave_sum(acc[k][0]);
      const double s1 = wave_sum(acc[k][1]);
      const double s2 = wave_sum(acc[k][2]);
      // K == 1: every lane mirrors star 0, so the chain state stays
      // wave-uniform and the fixed-point loops never diverge.
      if (MAXK == 1 || lane == k) {
        gf = -s0;
        gx = -s1 * f / c.var;
        gy = -s2 * f / c.var;
      }
    }
  }
  if (c.use_prior) gf += c.alpha / f;  // :408-409
  if (c.use_Vc) {                      // :411-418 (O(K^2), lanes = stars)
    double sx = 0.0, sy = 0.0;
    for (int jj = 0; jj < K; ++jj) {
      const double X = bcast(x, jj), Y = bcast(y, jj);
      const double ddx = X - x, ddy = Y - y;
      double R = sqrt(ddx * ddx + ddy * ddy);
      if (fabs(R) < 1e-10) R = 1e32;
      const double tr = pow(1.0 / R, c.vc_pow + 2.0);
      sx += tr * ddx;
      sy += tr * ddy;
    }
    gx += c.beta * sx * c.vc_pow;
    gy += c.beta * sy * c.vc_pow;
  }
  if (with_metric) gf += metric_flux_term(f, c);  // dphidq (:459-463)
  // Tables are rebuilt by the next gradient call; make sure every lane has
  // finished reading before they are overwritten.
  wave_lds_sync();
}

struct LeapArgs {
  double* q;
  double* p;
  int32_t* fp_iters;
  int32_t* status;
  const double* D;
  int64_t n_chains;
  int K, n_steps;
  Geometry g;
  Consts c;
  // ragged sets (rhmc_leapfrog_ragged_device): chain
  // i is row rows[i] (NULL: row i) of [*][ld] arrays with Kc[row] stars; K is
  // then the largest star count of the launch (it sizes LDS).  Kc NULL: every
  // chain has K stars in rows of 3K.
  const int32_t* Kc = nullptr;
  const int64_t* rows = nullptr;
  int64_t ld = 0;
};

// Row, star count and row stride of launch chain i (LeapArgs / EnergyArgs).
template <class A>
__device__ __forceinline__ void chain_row(const A& a, int64_t i, int64_t& row, int& K,
                                          int64_t& ld) {
  row = a.rows ? a.rows[i] : i;
  K = a.Kc ? a.Kc[row] : a.K;
  ld = a.Kc ? a.ld : 3 * (int64_t)K;
}

// Stage D into LDS (coalesced, whole workgroup) and return this wave's chain.
__device__ __forceinline__ int64_t stage_image(double* sD, const double* __restrict__ D,
                                               int npix, int waves_per_wg) {
  for (int e = threadIdx.x; e < npix; e += blockDim.x) sD[e] = D[e];
  __syncthreads();
  return (int64_t)blockIdx.x * waves_per_wg + (threadIdx.x / kWave);
}

// Gradient policy of the slotted kernels on the image in LDS (the plan's
// Family::LdsImage, K <= MAXK <= 16, any PSF width): D staged once per
// workgroup, behind it one region of separable tables per wave, sized by the
// launch's K and laid out by the chain's (ragged sets).  One slot; `lc` unused.
template <int MAXK>
struct LdsG {
  static __host__ __device__ constexpr size_t lds_bytes(int waves, int K, int rows, int cols) {
    return ((size_t)rows * cols + waves * table_doubles(K, rows, cols)) * sizeof(double);
  }
  struct Ctx {
    const double* sD;  // LDS [npix]
    double* tab;       // this wave's table region
    Geometry g;
  };
  static __device__ __forceinline__ Ctx setup(double* lds, const double* D, int K,
                                              const Geometry& g) {
    stage_image(lds, D, g.npix, blockDim.x / kWave);
    return Ctx{lds, lds + g.npix + (threadIdx.x / kWave) * table_doubles(K, g.rows, g.cols), g};
  }
  template <int SLOTS>
  static __device__ __forceinline__ void gradient(const Ctx& g, int K, const double (&f)[SLOTS],
                                                  const double (&x)[SLOTS],
                                                  const double (&y)[SLOTS], const Consts& c,
                                                  const LeanConsts&, bool with_metric,
                                                  double (&gf)[SLOTS], double (&gx)[SLOTS],
                                                  double (&gy)[SLOTS]) {
    static_assert(SLOTS == 1, "lane k < K <= 16 owns star k");
    rhmc::gradient<MAXK>(g.sD, carve_tables(g.tab, K, g.g), K, f[0], x[0], y[0], g.g, c,
                         with_metric, gf[0], gx[0], gy[0]);
  }
  // sum over pixels of Lambda - D log Lambda (sampler_RHMC.py:319-327)
  template <int SLOTS>
  static __device__ __forceinline__ double potential(const Ctx& g, int K,
                                                     const double (&f)[SLOTS],
                                                     const double (&x)[SLOTS],
                                                     const double (&y)[SLOTS], const Consts& c,
                                                     const LeanConsts&) {
    static_assert(SLOTS == 1, "lane k < K <= 16 owns star k");
    const Geometry& geo = g.g;
    const Tables tab = carve_tables(g.tab, K, geo);
    const int lane = lane_id();
    build_tables(tab, K, x[0], y[0], geo, c);
    double fk[MAXK];
#pragma unroll
    for (int k = 0; k < MAXK; ++k) fk[k] = (k < K) ? bcast(f[0], k) : 0.0;
    double v = 0.0;
    int i = lane / geo.cols, j = lane - (lane / geo.cols) * geo.cols;
    for (int tt = 0; tt < geo.npl; ++tt) {
      const int pix = lane + kWave * tt;
      if (pix < geo.npix) {
        double lam = c.B;
#pragma unroll
        for (int k = 0; k < MAXK; ++k)
          if (k < K) lam = fma(fk[k], tab.ex[k * geo.rows + i] * tab.ey[k * geo.cols + j], lam);
        v += lam - g.sD[pix] * log(lam);
      }
      j += geo.dj;
      i += geo.di;
      if (j >= geo.cols) {
        j -= geo.cols;
        ++i;
      }
    }
    return wave_sum(v);
  }
};

// Chain state of one wave: lane k < K owns star k (UNIFORM: K == 1 and every
// lane mirrors star 0, so no cross-lane reduction is needed).
struct StarState {
  double f, x, y, pf, px, py;
};

// n_steps implicit generalized-leapfrog steps (sampler_RHMC.py:522-566) with a
// single gradient call site: the end-of-step gradient (:551) is the next
// step's opening one (:525).  `grad(f, x, y, gf, gx, gy)` returns dphidq.
template <bool UNIFORM, class Grad>
__device__ __forceinline__ void run_steps(StarState& s, bool owner, int n_steps, int rows,
                                          int cols, const Consts& c, int& it_p, int& it_q,
                                          unsigned& st, Grad grad) {
  const double hdt = c.hdt;
  for (int step = 0;; ++step) {
    double gf, gx, gy;
    grad(s.f, s.x, s.y, gf, gx, gy);
    if (step > 0) {
      // (5) closing half kick of the previous step (:551), (6) reflection (:554-564)
      s.pf = s.pf - hdt * gf;
      s.px = s.px - hdt * gx;
      s.py = s.py - hdt * gy;
      if (s.f < c.f_lim) {
        s.pf = -s.pf;
        st |= RHMC_STATUS_REFLECT_F;
        if (s.f >= c.near_f) st |= RHMC_STATUS_NEAR_WALL;
      }
      if (s.x < 0.0 || s.x > (double)(rows - 1)) {
        s.px = -s.px;
        st |= RHMC_STATUS_REFLECT_XY;
        if (near_edge(s.x, (double)(rows - 1))) st |= RHMC_STATUS_NEAR_WALL;
      }
      if (s.y < 0.0 || s.y > (double)(cols - 1)) {
        s.py = -s.py;
        st |= RHMC_STATUS_REFLECT_XY;
        if (near_edge(s.y, (double)(cols - 1))) st |= RHMC_STATUS_NEAR_WALL;
      }
    }
    if (step == n_steps) break;
    // (1) opening half kick (:525)
    s.pf = s.pf - hdt * gf;
    s.px = s.px - hdt * gx;
    s.py = s.py - hdt * gy;
    // (2) p fixed point, flux slots only (:528-535); x/y slots change by 0
    {
      const double coef = dtaudq_coef(s.f, c);
      const double rho = s.pf;
      double dp;
      int n = 0;
      do {
        const double pp = rho - hdt * ((s.pf * s.pf) * coef / 2.0);
        const double d = (UNIFORM || owner) ? fabs(s.pf - pp) : 0.0;
        dp = UNIFORM ? d : wave_nanmax(d);
        s.pf = pp;
        ++n;
      } while (dp > c.delta && n < c.counter_max);
      it_p += n;
      if (dp > c.delta) st |= RHMC_STATUS_PLOOP_CAP;
    }
    // (3) q fixed point (:538-545): q' = sig + dt/2 (p/H(sig) + p/H(q))
    {
      const double sf = s.f, sx = s.x, sy = s.y;
      const double hff0 = H_ff(sf, c), hxx0 = H_xx(sf, c);
      const double af = s.pf / hff0, ax = s.px / hxx0, ay = s.py / hxx0;
      double dq;
      int n = 0;
      do {
        const double hff = H_ff(s.f, c), hxx = H_xx(s.f, c);
        const double nf = sf + hdt * (af + s.pf / hff);
        const double nx = sx + hdt * (ax + s.px / hxx);
        const double ny = sy + hdt * (ay + s.py / hxx);
        double d = nanmax2(nanmax2(fabs(s.f - nf), fabs(s.x - nx)), fabs(s.y - ny));
        d = (UNIFORM || owner) ? d : 0.0;
        dq = UNIFORM ? d : wave_nanmax(d);
        s.f = nf;
        s.x = nx;
        s.y = ny;
        ++n;
      } while (dq > c.delta && n < c.counter_max);
      it_q += n;
      if (dq > c.delta) st |= RHMC_STATUS_QLOOP_CAP;
    }
    // (4) p -= dt/2 dtaudq(q, p) (:548)
    s.pf = s.pf - hdt * ((s.pf * s.pf) * dtaudq_coef(s.f, c) / 2.0);
  }
}

__device__ __forceinline__ StarState load_chain(const LeapArgs& a, int64_t chain, int K,
                                                bool owner, int64_t& base) {
  base = chain * 3 * (int64_t)K + 3 * (owner ? lane_id() : 0);
  StarState s;
  s.f = a.q[base];
  s.x = a.q[base + 1];
  s.y = a.q[base + 2];
  s.pf = a.p[base];
  s.px = a.p[base + 1];
  s.py = a.p[base + 2];
  return s;
}

__device__ __forceinline__ void store_chain(const LeapArgs& a, int64_t chain, int64_t base,
                                            bool owner, const StarState& s, int it_p, int it_q,
                                            unsigned st) {
  if (owner) {
    if (!(isfinite(s.f) && isfinite(s.x) && isfinite(s.y) && isfinite(s.pf) &&
          isfinite(s.px) && isfinite(s.py)))
      st |= RHMC_STATUS_NONFINITE;
    a.q[base] = s.f;
    a.q[base + 1] = s.x;
    a.q[base + 2] = s.y;
    a.p[base] = s.pf;
    a.p[base + 1] = s.px;
    a.p[base + 2] = s.py;
  }
  // OR the star lanes' status bits
  unsigned all = owner ? st : 0u;
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) all |= (unsigned)__shfl_xor((int)all, m, kWave);
  if (lane_id() == 0) {
    if (a.status) a.status[chain] = (int32_t)all;
    if (a.fp_iters) {
      a.fp_iters[2 * chain] = it_p;
      a.fp_iters[2 * chain + 1] = it_q;
    }
  }
}

// Generic kernel: image in LDS, K <= MAXK <= 16, reference-form metric.
template <int MAXK>
__global__ void __launch_bounds__(256) leapfrog_kernel(LeapArgs a) {
  extern __shared__ double lds[];
  const Geometry& g = a.g;
  const Consts& c = a.c;
  const int W = blockDim.x / kWave;
  double* sD = lds;
  const int64_t chain = stage_image(sD, a.D, g.npix, W);
  if (chain >= a.n_chains) return;
  const int K = a.K;
  const Tables tab = carve_tables(
      lds + g.npix + (threadIdx.x / kWave) * table_doubles(K, g.rows, g.cols), K, g);
  const bool owner = lane_id() < K;
  int64_t base;
  StarState s = load_chain(a, chain, K, owner, base);
  int it_p = 0, it_q = 0;
  unsigned st = 0u;
  run_steps<MAXK == 1>(s, owner, a.n_steps, g.rows, g.cols, c, it_p, it_q, st,
                       [&](double f, double x, double y, double& gf, double& gx, double& gy) {
                         gradient<MAXK>(sD, tab, K, f, x, y, g, c, true, gf, gx, gy);
                       });
  store_chain(a, chain, base, owner, s, it_p, it_q, st);
}

// ---------------------------------------------------------------------------
// The slotted frame: one wave per chain, star 64 s + lane in register slot s
// (SLOTS = 1 for LdsG's energy and gradient; 1, 2, 4 for the windowed and dense
// policies up to 256 stars; WinGG to 16).
template <int SLOTS>
struct WinState {
  double f[SLOTS], x[SLOTS], y[SLOTS], pf[SLOTS], px[SLOTS], py[SLOTS];
  bool own[SLOTS];
};

// Lanes without a star in a slot carry a copy of star 0 (finite, never read).
// The chain's stars start at element row * ld of q and p.
template <int SLOTS>
__device__ __forceinline__ void win_load(const LeapArgs& a, int64_t row, int64_t ld, int K,
                                         WinState<SLOTS>& s) {
  const int lane = lane_id();
#pragma unroll
  for (int t = 0; t < SLOTS; ++t) {
    s.own[t] = kWave * t + lane < K;
    const int64_t e = row * ld + 3 * (s.own[t] ? kWave * t + lane : 0);
    s.f[t] = a.q[e];
    s.x[t] = a.q[e + 1];
    s.y[t] = a.q[e + 2];
    s.pf[t] = a.p[e];
    s.px[t] = a.p[e + 1];
    s.py[t] = a.p[e + 2];
  }
}

template <int SLOTS>
__device__ __forceinline__ void win_store(const LeapArgs& a, int64_t chain, int64_t row,
                                          int64_t ld, int K, const WinState<SLOTS>& s, int it_p,
                                          int it_q, unsigned st) {
  const int lane = lane_id();
#pragma unroll
  for (int t = 0; t < SLOTS; ++t) {
    if (!s.own[t]) continue;
    if (!(isfinite(s.f[t]) && isfinite(s.x[t]) && isfinite(s.y[t]) && isfinite(s.pf[t]) &&
          isfinite(s.px[t]) && isfinite(s.py[t])))
      st |= RHMC_STATUS_NONFINITE;
    const int64_t e = row * ld + 3 * (kWave * t + lane);
    a.q[e] = s.f[t];
    a.q[e + 1] = s.x[t];
    a.q[e + 2] = s.y[t];
    a.p[e] = s.pf[t];
    a.p[e + 1] = s.px[t];
    a.p[e + 2] = s.py[t];
  }
  unsigned all = s.own[0] ? st : 0u;  // status bits are only set for owned slots
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) all |= (unsigned)__shfl_xor((int)all, m, kWave);
  if (lane == 0) {
    if (a.status) a.status[chain] = (int32_t)all;
    if (a.fp_iters) {
      a.fp_iters[2 * chain] = it_p;
      a.fp_iters[2 * chain + 1] = it_q;
    }
  }
}

// n_steps RHMC_single_step()s (sampler_RHMC.py:522-566) on the slotted state,
// the reference-form metric of run_steps; the fixed-point tests take np.max
// over all 3K coordinates (NaN propagates) with one wave max per iteration.
template <int SLOTS, class Grad>
__device__ __forceinline__ void run_steps_win(WinState<SLOTS>& s, int n_steps, int rows,
                                              int cols, const Consts& c, int& it_p, int& it_q,
                                              unsigned& st, Grad grad) {
  const double hdt = c.hdt;
  for (int step = 0;; ++step) {
    double gf[SLOTS], gx[SLOTS], gy[SLOTS];
    grad(s.f, s.x, s.y, gf, gx, gy);
    if (step > 0) {
#pragma unroll
      for (int t = 0; t < SLOTS; ++t) {
        // (5) closing half kick of the previous step (:551), (6) reflection (:554-564)
        s.pf[t] = s.pf[t] - hdt * gf[t];
        s.px[t] = s.px[t] - hdt * gx[t];
        s.py[t] = s.py[t] - hdt * gy[t];
        unsigned b = 0u;
        if (s.f[t] < c.f_lim) {
          s.pf[t] = -s.pf[t];
          b |= RHMC_STATUS_REFLECT_F;
          if (s.f[t] >= c.near_f) b |= RHMC_STATUS_NEAR_WALL;
        }
        if (s.x[t] < 0.0 || s.x[t] > (double)(rows - 1)) {
          s.px[t] = -s.px[t];
          b |= RHMC_STATUS_REFLECT_XY;
          if (near_edge(s.x[t], (double)(rows - 1))) b |= RHMC_STATUS_NEAR_WALL;
        }
        if (s.y[t] < 0.0 || s.y[t] > (double)(cols - 1)) {
          s.py[t] = -s.py[t];
          b |= RHMC_STATUS_REFLECT_XY;
          if (near_edge(s.y[t], (double)(cols - 1))) b |= RHMC_STATUS_NEAR_WALL;
        }
        if (s.own[t]) st |= b;
      }
    }
    if (step == n_steps) break;
#pragma unroll
    for (int t = 0; t < SLOTS; ++t) {  // (1) opening half kick (:525)
      s.pf[t] = s.pf[t] - hdt * gf[t];
      s.px[t] = s.px[t] - hdt * gx[t];
      s.py[t] = s.py[t] - hdt * gy[t];
    }
    {  // (2) p fixed point, flux slots only (:528-535); x/y slots change by 0
      double coef[SLOTS], rho[SLOTS];
#pragma unroll
      for (int t = 0; t < SLOTS; ++t) {
        coef[t] = dtaudq_coef(s.f[t], c);
        rho[t] = s.pf[t];
      }
      double dp;
      int n = 0;
      do {
        double d = 0.0;
#pragma unroll
        for (int t = 0; t < SLOTS; ++t) {
          const double pp = rho[t] - hdt * ((s.pf[t] * s.pf[t]) * coef[t] / 2.0);
          const double dd = s.own[t] ? fabs(s.pf[t] - pp) : 0.0;
          d = t == 0 ? dd : nanmax2(d, dd);
          s.pf[t] = pp;
        }
        dp = wave_nanmax(d);
        ++n;
      } while (dp > c.delta && n < c.counter_max);
      it_p += n;
      if (dp > c.delta) st |= RHMC_STATUS_PLOOP_CAP;
    }
    {  // (3) q fixed point (:538-545): q' = sig + dt/2 (p/H(sig) + p/H(q))
      double sf[SLOTS], sx[SLOTS], sy[SLOTS], af[SLOTS], ax[SLOTS], ay[SLOTS];
#pragma unroll
      for (int t = 0; t < SLOTS; ++t) {
        sf[t] = s.f[t];
        sx[t] = s.x[t];
        sy[t] = s.y[t];
        const double hff0 = H_ff(sf[t], c), hxx0 = H_xx(sf[t], c);
        af[t] = s.pf[t] / hff0;
        ax[t] = s.px[t] / hxx0;
        ay[t] = s.py[t] / hxx0;
      }
      double dq;
      int n = 0;
      do {
        double d = 0.0;
#pragma unroll
        for (int t = 0; t < SLOTS; ++t) {
          const double hff = H_ff(s.f[t], c), hxx = H_xx(s.f[t], c);
          const double nf = sf[t] + hdt * (af[t] + s.pf[t] / hff);
          const double nx = sx[t] + hdt * (ax[t] + s.px[t] / hxx);
          const double ny = sy[t] + hdt * (ay[t] + s.py[t] / hxx);
          double dd =
              nanmax2(nanmax2(fabs(s.f[t] - nf), fabs(s.x[t] - nx)), fabs(s.y[t] - ny));
          dd = s.own[t] ? dd : 0.0;
          d = t == 0 ? dd : nanmax2(d, dd);
          s.f[t] = nf;
          s.x[t] = nx;
          s.y[t] = ny;
        }
        dq = wave_nanmax(d);
        ++n;
      } while (dq > c.delta && n < c.counter_max);
      it_q += n;
      if (dq > c.delta) st |= RHMC_STATUS_QLOOP_CAP;
    }
#pragma unroll
    for (int t = 0; t < SLOTS; ++t)  // (4) p -= dt/2 dtaudq(q, p) (:548)
      s.pf[t] = s.pf[t] - hdt * ((s.pf[t] * s.pf[t]) * dtaudq_coef(s.f[t], c) / 2.0);
  }
}


// Leapfrog on the slotted state (1 <= K <= 64 SLOTS) with gradient policy G:
// WinG (windowed, any square image, D from global memory) or DenseG<IMG>
// (rhmc_dense.hpp: 32/48-px images, many stars).
template <class G, int SLOTS>
__global__ void __launch_bounds__(256) leapfrog_win_kernel(LeapArgs a) {
  extern __shared__ double lds[];
  const typename G::Ctx gctx = G::setup(lds, a.D, a.K, a.g);
  const Consts& c = a.c;
  const int W = blockDim.x / kWave;
  const int64_t chain = (int64_t)blockIdx.x * W + (threadIdx.x / kWave);
  if (chain >= a.n_chains) return;
  int64_t row, ld;
  int K;
  chain_row(a, chain, row, K, ld);
  const LeanConsts lc = lean_consts(c);
  WinState<SLOTS> s;
  win_load<SLOTS>(a, row, ld, K, s);
  int it_p = 0, it_q = 0;
  unsigned st = 0u;
  const int rows = a.g.rows, cols = a.g.cols;
  run_steps_win<SLOTS>(
      s, a.n_steps, rows, cols, c, it_p, it_q, st,
      [&](const double(&f)[SLOTS], const double(&x)[SLOTS], const double(&y)[SLOTS],
          double(&gf)[SLOTS], double(&gx)[SLOTS], double(&gy)[SLOTS]) {
        G::template gradient<SLOTS>(gctx, K, f, x, y, c, lc, true, gf, gx, gy);
      });
  win_store<SLOTS>(a, chain, row, ld, K, s, it_p, it_q, st);
}

struct GradArgs {
  const double* q;
  double* grad;
  const double* D;
  int64_t n_chains;
  int K, with_metric;
  Geometry g;
  Consts c;
};

struct EnergyArgs {
  const double* q;
  const double* p;
  double* V;
  double* T;
  const double* D;
  int64_t n_chains;
  int K, f_pos;
  Geometry g;
  Consts c;
  // ragged sets (rhmc_energy_ragged_device), as LeapArgs
  const int32_t* Kc = nullptr;
  const int64_t* rows = nullptr;
  int64_t ld = 0;
};

// ---------------------------------------------------------------------------
// Alternative integrators, windowed gradient, lanes = stars:
//   HMC:        single_gym.run_single_HMC leapfrog, unit metric (:628-645)
//   RHMC_NAIVE: run_single_RHMC solver="naive"     (:690-708)
//   RHMC_LF:    run_single_RHMC solver="leap_frog" (:709-728)
// The loop is explicit_steps (rhmc_traj.hpp); this family's metric view divides
// by H_ff and H_xx at the slot's flux.
struct WinMetricView {
  // a copy, not a reference, on purpose: the drifts of x and y divide at the
  // flux before the step's drift, after f[t] has already been updated
  double f;
  const Consts& c;
  __device__ __forceinline__ double over_Hff(double v) const { return v / H_ff(f, c); }
  __device__ __forceinline__ double over_Hxx(double v) const { return v / H_xx(f, c); }
  // dVdq_RHMC (:427-446): flux slot ((p_f^2 (-H_ff'/H_ff^2)) + H_ff'/H_ff + 2 H_xx'/H_xx)/2.
  __device__ __forceinline__ double force_f(double pf) const {
    const double hff = H_ff(f, c), hffg = H_ff_grad(f, c);
    const double hxx = H_xx(f, c), hxxg = H_xx_grad(f, c);
    const double t1 = (pf * pf) * (-hffg / (hff * hff));
    const double t2 = (hffg / hff) + (2.0 * hxxg / hxx);
    return (t1 + t2) / 2.0;
  }
};

template <class G, int SOLVER, int SLOTS>
__global__ void __launch_bounds__(256) integrate_win_kernel(LeapArgs a, int f_pos) {
  extern __shared__ double lds[];
  const typename G::Ctx gctx = G::setup(lds, a.D, a.K, a.g);
  const Consts& c = a.c;
  const int W = blockDim.x / kWave;
  const int64_t chain = (int64_t)blockIdx.x * W + (threadIdx.x / kWave);
  if (chain >= a.n_chains) return;
  const int K = a.K;
  const LeanConsts lc = lean_consts(c);
  WinState<SLOTS> s;
  win_load<SLOTS>(a, chain, 3 * (int64_t)K, K, s);
  unsigned st = 0u;
  explicit_steps<SOLVER, SLOTS>(
      s.f, s.x, s.y, s.pf, s.px, s.py, a.n_steps, f_pos, c.f_lim, c.dt, st,
      [&](double (&gf)[SLOTS], double (&gx)[SLOTS], double (&gy)[SLOTS]) RHMC_INLINE_LAMBDA {
        G::template gradient<SLOTS>(gctx, K, s.f, s.x, s.y, c, lc, false, gf, gx, gy);
#pragma unroll
        // + dVdq_RHMC's zero position slots, for every kick (HMC's first half
        // kick once went without: that differs only in the sign of a zero, when
        // the gradient and the momentum are both exactly -0.0)
        for (int t = 0; t < SLOTS; ++t) {
          gx[t] = gx[t] + 0.0;
          gy[t] = gy[t] + 0.0;
        }
      },
      [&](int t) RHMC_INLINE_LAMBDA { return WinMetricView{s.f[t], c}; },
      [&](int t) RHMC_INLINE_LAMBDA { return s.own[t]; }, [] {});
  win_store<SLOTS>(a, chain, chain, 3 * (int64_t)K, K, s, 0, 0, st);
}

// samplers.lightsource_gym.HMC_random's trajectory (samplers.py:519-552), or
// with DIAG RHMC_random_diag's (:766-800): random_trajectory (rhmc_traj.hpp,
// the rule and the reference's wall quirks) on the slotted gradient.  One wave
// per chain, star 64 t + lane in slot t; the steps dtv[3K] sit in registers,
// and s.p* keep the start momentum for the DIAG force and the REFLECT_F return.
template <class G, int SLOTS, bool DIAG>
__device__ __forceinline__ void hmc_random_win_body(double* lds, const LeapArgs& a,
                                                    const double* __restrict__ dtv,
                                                    const int32_t* __restrict__ steps,
                                                    const DiagArgs& dg) {
  const typename G::Ctx gctx = G::setup(lds, a.D, a.K, a.g);
  const Consts& c = a.c;
  const int W = blockDim.x / kWave;
  const int64_t chain = (int64_t)blockIdx.x * W + (threadIdx.x / kWave);
  if (chain >= a.n_chains) return;
  const int K = a.K;
  const LeanConsts lc = lean_consts(c);
  const int lane = lane_id();
  WinState<SLOTS> s;
  win_load<SLOTS>(a, chain, 3 * (int64_t)K, K, s);
  double dtr[SLOTS][3];
  if constexpr (!DIAG) {
#pragma unroll
    for (int t = 0; t < SLOTS; ++t) {
      const int ks = s.own[t] ? kWave * t + lane : 0;
#pragma unroll
      for (int j = 0; j < 3; ++j) dtr[t][j] = dtv[3 * ks + j];
    }
  }
  double hf[SLOTS], hx[SLOTS], hy[SLOTS];
#pragma unroll
  for (int t = 0; t < SLOTS; ++t) {
    hf[t] = s.pf[t];
    hx[t] = s.px[t];
    hy[t] = s.py[t];
  }
  const bool flip = random_trajectory<SLOTS, DIAG>(
      s.f, s.x, s.y, hf, hx, hy, steps[chain], c.f_lim, dg,
      [&](int t, int j) RHMC_INLINE_LAMBDA { return dtr[t][j]; },
      [&](int t) RHMC_INLINE_LAMBDA { return s.own[t]; },
      [&](bool b) RHMC_INLINE_LAMBDA { return __builtin_amdgcn_ballot_w64(b) != 0; },
      [&](double (&gf)[SLOTS], double (&gx)[SLOTS], double (&gy)[SLOTS]) RHMC_INLINE_LAMBDA {
        G::template gradient<SLOTS>(gctx, K, s.f, s.x, s.y, c, lc, false, gf, gx, gy);
      },
      [&](int t, double& sf, double& sxy) RHMC_INLINE_LAMBDA {
        sf = s.pf[t] * s.pf[t];
        sxy = s.px[t] * s.px[t] + s.py[t] * s.py[t];
      },
      [&](int row) RHMC_INLINE_LAMBDA {
        if (!dg.trace || row >= dg.rows) return;
#pragma unroll
        for (int t = 0; t < SLOTS; ++t) {
          if (!s.own[t]) continue;
          double* r = dg.trace + (chain * dg.rows + row) * 3 * K + 3 * (kWave * t + lane);
          r[0] = s.f[t];
          r[1] = s.x[t];
          r[2] = s.y[t];
        }
      });
  unsigned st = 0u;
  if (flip) {
    st |= RHMC_STATUS_REFLECT_F;  // s.p* stay the starting momentum
  } else {
#pragma unroll
    for (int t = 0; t < SLOTS; ++t) {
      s.pf[t] = hf[t];
      s.px[t] = hx[t];
      s.py[t] = hy[t];
    }
  }
  win_store<SLOTS>(a, chain, chain, 3 * (int64_t)K, K, s, 0, 0, st);
}

template <class G, int SLOTS>
__global__ void __launch_bounds__(256) hmc_random_win_kernel(LeapArgs a,
                                                             const double* __restrict__ dtv,
                                                             const int32_t* __restrict__ steps) {
  extern __shared__ double lds[];
  hmc_random_win_body<G, SLOTS, false>(lds, a, dtv, steps, DiagArgs{});
}

// The DIAG body (rhmc_diag_random).
template <class G, int SLOTS>
__global__ void __launch_bounds__(256) diag_hmc_random_win_kernel(
    LeapArgs a, const int32_t* __restrict__ steps, DiagArgs dg) {
  extern __shared__ double lds[];
  hmc_random_win_body<G, SLOTS, true>(lds, a, nullptr, steps, dg);
}

// Star 64 t + lane's (f, x, y) of a chain (lanes without a star: star 0's).
template <int SLOTS>
__device__ __forceinline__ void win_load_q(const double* q, int64_t row, int64_t ld, int K,
                                           double (&f)[SLOTS], double (&x)[SLOTS],
                                           double (&y)[SLOTS], bool (&own)[SLOTS]) {
#pragma unroll
  for (int t = 0; t < SLOTS; ++t) {
    own[t] = win_own(t, K);
    const int64_t e = row * ld + 3 * (own[t] ? kWave * t + lane_id() : 0);
    f[t] = q[e];
    x[t] = q[e + 1];
    y[t] = q[e + 2];
  }
}

// dVdq or dphidq of policy G, one wave per chain.
template <class G, int SLOTS>
__global__ void __launch_bounds__(256) gradient_win_kernel(GradArgs a) {
  extern __shared__ double lds[];
  const typename G::Ctx gctx = G::setup(lds, a.D, a.K, a.g);
  const int W = blockDim.x / kWave;
  const int64_t chain = (int64_t)blockIdx.x * W + (threadIdx.x / kWave);
  if (chain >= a.n_chains) return;
  const int K = a.K;
  const LeanConsts lc = lean_consts(a.c);
  double f[SLOTS], x[SLOTS], y[SLOTS], gf[SLOTS], gx[SLOTS], gy[SLOTS];
  bool own[SLOTS];
  win_load_q<SLOTS>(a.q, chain, 3 * (int64_t)K, K, f, x, y, own);
  G::template gradient<SLOTS>(gctx, K, f, x, y, a.c, lc, a.with_metric != 0, gf, gx, gy);
#pragma unroll
  for (int t = 0; t < SLOTS; ++t) {
    if (!own[t]) continue;
    const int64_t e = chain * 3 * (int64_t)K + 3 * (kWave * t + lane_id());
    a.grad[e] = gf[t];
    a.grad[e + 1] = gx[t];
    a.grad[e + 2] = gy[t];
  }
}

// V (sampler_RHMC.py:294-351) and T at H(q) (:353-363), one wave per chain:
// the policy's potential, the rest here.  Ragged sets (a.Kc): the chain's row
// and star count; the policy's setup sees the set's largest K (a.K).
template <class G, int SLOTS>
__global__ void __launch_bounds__(256) energy_win_kernel(EnergyArgs a) {
  extern __shared__ double lds[];
  const typename G::Ctx gctx = G::setup(lds, a.D, a.K, a.g);
  const Geometry& g = a.g;
  const Consts& c = a.c;
  const int W = blockDim.x / kWave;
  const int64_t chain = (int64_t)blockIdx.x * W + (threadIdx.x / kWave);
  if (chain >= a.n_chains) return;
  const int lane = lane_id();
  int64_t row, ld;
  int K;
  chain_row(a, chain, row, K, ld);
  const LeanConsts lc = lean_consts(c);
  double f[SLOTS], x[SLOTS], y[SLOTS];
  bool own[SLOTS];
  win_load_q<SLOTS>(a.q, row, ld, K, f, x, y, own);
  if (a.T) {
    double t1 = 0.0, t2 = 0.0;
#pragma unroll
    for (int t = 0; t < SLOTS; ++t) {
      if (!own[t]) continue;
      const int64_t e = row * ld + 3 * (kWave * t + lane);
      const double pf = a.p[e], px = a.p[e + 1], py = a.p[e + 2];
      const double hff = H_ff(f[t], c), hxx = H_xx(f[t], c);
      t1 += pf * pf / hff + px * px / hxx + py * py / hxx;
      t2 += log(fabs(hff)) + log(fabs(hxx)) + log(fabs(hxx));
    }
    t1 = wave_sum(t1);
    t2 = wave_sum(t2);
    if (lane == 0) a.T[chain] = (t1 + t2) / 2.0;
  }
  if (!a.V) return;
  bool bad = false;
#pragma unroll
  for (int t = 0; t < SLOTS; ++t) {
    if (!own[t]) continue;
    if ((a.f_pos & RHMC_V_FLUX_WALL) && f[t] < c.f_lim) bad = true;
    if (!(a.f_pos & RHMC_V_NO_POSCHECK) &&
        (x[t] < -1.0 || x[t] > (double)(g.rows + 1) || y[t] < -1.0 ||
         y[t] > (double)(g.cols + 1)))
      bad = true;
  }
  if (__any(bad)) {
    if (lane == 0) a.V[chain] = INFINITY;
    return;
  }
  double v = G::template potential<SLOTS>(gctx, K, f, x, y, c, lc);
  if (c.use_prior) {
    double vp = 0.0;
#pragma unroll
    for (int t = 0; t < SLOTS; ++t)
      if (own[t]) vp += c.alpha * log(f[t]) + c.vprior;
    v += wave_sum(vp);
  }
  if (c.use_Vc) {  // 0.5 beta sum_{a,b} R_ab^-pow with R_aa -> 1e32 (:332-349)
    double sl = 0.0;
#pragma unroll
    for (int t = 0; t < SLOTS; ++t) {
      double sv = 0.0;
#pragma unroll
      for (int t2 = 0; t2 < SLOTS; ++t2) {
        for (int jl = 0; jl < kWave && kWave * t2 + jl < K; ++jl) {
          const double X = bcast(x[t2], jl), Y = bcast(y[t2], jl);
          double R = sqrt((X - x[t]) * (X - x[t]) + (Y - y[t]) * (Y - y[t]));
          if (fabs(R) < 1e-10) R = 1e32;
          sv += pow(1.0 / R, c.vc_pow);
        }
      }
      if (own[t]) sl += sv;
    }
    v += 0.5 * c.beta * wave_sum(sl);
  }
  if (lane == 0) a.V[chain] = v;
}

}  // namespace rhmc
