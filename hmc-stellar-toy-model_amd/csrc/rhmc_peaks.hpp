// rhmc_peaks.hpp — samplers.lightsource_gym.find_peaks' seed descent
// (samplers.py:190-221) on the GPU: every seed runs up to n_step steps of
// gradient descent on the one-star potential V_single (:121-127) against the
// pure-background model, with the reference's three ways to stop:
//
//   V_prev = V(f, x, y)
//   for i in 0 .. n_step-1:
//     (gf, gx, gy) = dVdq_single(f, x, y)               (:93-101)
//     dt_f = f dt_f_coeff ; dt_xy = dt_xy_coeff / f     (:201-202, f before the update)
//     f -= gf dt_f ; x -= gx dt_xy ; y -= gy dt_xy      (:205-207)
//     f < f_lim                          -> FAINT       (:209-211)
//     V_cur = V(f, x, y)
//     |(V_cur - V_prev) / V_prev| < tol  -> CONVERGED   (:215-216)
//     V_prev = V_cur
//   else                                 -> CAP
//
// peaks_k1_tiledr: the whole descent in one launch on the one-star
// register-window layout (rhmc_tiledr.hpp: 16 lanes per seed, 4 seeds per
// wave64, image and exp table in LDS, the 28-px window's pixels in registers).
// After an update V_cur and the next step's gradient are taken at the same
// (f, x, y), so ONE pass over the lane's 49 cached pixels (peaks_pass) gives
// Lambda, the window's part of V and the three gradient sums from one set of
// PSF factors and one window check.  V = sum_image (B - D ln B) + the window's
// (Lambda - B) - D (ln Lambda - ln B), with log_pos on both sides of the
// difference (rhmc_mhk1.hpp).
//
// Seeds of one wave stop at different steps.  The step loop has the trip count
// n_step and leaves early only on a wave-wide ballot; a finished seed's lanes
// keep executing and freeze their state with selects, so the window check and
// every DPP / swizzle / bpermute run with all 64 lanes.
//
// peaks_update_kernel: the same recurrence one step at a time for the
// configurations the fused kernel does not take (other image sides, wide
// PSFs, forced per-wave families): the library's K = 1 gradient and energy
// launches evaluate dVdq and V on device arrays and this kernel, one thread
// per seed, applies the update, the two tests, the step count and the status
// between them.
#pragma once
#include "rhmc_mhk1.hpp"
#include "rhmc_tiledr.hpp"

namespace rhmc {

struct PeaksArgs {
  double* q;              // [n][3] seeds (f, x, y), updated in place
  int32_t* steps;         // nullable [n]: gradient evaluations
  int32_t* status;        // nullable [n]: RHMC_PEAK_* | RHMC_STATUS_NONFINITE
  double* V;              // nullable [n]: the last V evaluated
  const double* D;
  const float* Df;        // D in fp32 when exact, else nullptr
  int64_t n;
  double f_lim, dt_f_coeff, dt_xy_coeff, rel_tol;
  int n_step, pad;
  Consts c;
};

// One step's update and faint test on one seed's scalars (both kernels).  In:
// the state and the gradient at it.  Out: the updated state; returns
// RHMC_PEAK_FAINT, or 0 when V has to be evaluated at the new state.
__device__ __forceinline__ unsigned peaks_update(double& f, double& x, double& y, double gf,
                                                 double gx, double gy, double dt_f_coeff,
                                                 double dt_xy_coeff, double f_lim) {
  const double dt_f = f * dt_f_coeff;              // :201
  const double dt_xy = dt_xy_coeff / f;            // :202
  f -= gf * dt_f;                                  // :205-207
  x -= gx * dt_xy;
  y -= gy * dt_xy;
  return f < f_lim ? RHMC_PEAK_FAINT : 0u;         // :209
}
__device__ __forceinline__ bool peaks_converged(double V_cur, double V_prev, double rel_tol) {
  return fabs((V_cur - V_prev) / V_prev) < rel_tol;  // :215 (NaN: false)
}

// The window's part of V (TiledR::potential_window) and the gradient
// (TiledR::partial / gradient) of one seed from one pass over its cached
// pixels.  Every lane of the seed's group gets all four values.
template <class TL, typename DT>
__device__ __forceinline__ void peaks_pass(const double* __restrict__ etab,
                                           const DT* __restrict__ sD,
                                           typename TL::Cache& k, double f, double x, double y,
                                           const Consts& c, const LeanConsts& lc, double lnB,
                                           double& vwin, double& gf, double& gx, double& gy) {
  constexpr int TR = TL::TR, TC = TL::TC;
  const int m = lane_id() % TL::LPC;
  const int a = m / 4, b = m % 4;
  double ex[TR], ey[TC];
  TL::ensure(sD, k, x, y);
  const double fs = flux_fold(f);
  TL::factors_rec(etab, k, x, y, lc, fs, ex, ey);  // ey carries fs
  // s_ij = D_ij / Lambda_ij - 1 (:88) into the separable row / column sums of
  // TiledR::partial; the same Lambda's log into the V correction.
  double R[TR], C[TC];
  double a0 = 0.0, a1 = 0.0, w1 = 0.0, v = 0.0;
#pragma unroll
  for (int i = 0; i < TR; ++i) {
#pragma unroll
    for (int j = 0; j < TC; ++j) {
      const double d = (double)k.d[i * TC + j];
      const double fp = ex[i] * ey[j];             // f PSF
      const double lam = fp + c.B;                 // Lambda (:85)
      double r = __builtin_amdgcn_rcp(lam);
      r = fma(r, fma(-lam, r, 1.0), r);
      const double sv = fma(d, r, -1.0);
      R[i] = (j == 0) ? ey[j] * sv : fma(ey[j], sv, R[i]);
      C[j] = (i == 0) ? ex[i] * sv : fma(ex[i], sv, C[j]);
      v += (lam - c.B) - d * (log_pos(lam) - lnB);
    }
    const double tt = ex[i] * R[i];
    a0 += tt;
    if (i > 0) a1 = fma(tt, (double)i, a1);
  }
#pragma unroll
  for (int j = 1; j < TC; ++j) w1 = fma(ey[j] * C[j], (double)(4 * j), w1);
  const double dxa = ((k.r0 + (double)(TR * a)) - x) + 0.5;  // lane's row 0 offset
  const double dyb = ((k.c0 + (double)b) - y) + 0.5;         // lane's column 0 offset
  const double s0 = TL::group_sum(a0);
  const double s1 = TL::group_sum(fma(dxa, a0, a1));
  const double s2 = TL::group_sum(fma(dyb, a0, w1));
  vwin = TL::group_sum(v);
  gf = -s0 * rcp_nr1(fs);                          // :94
  gx = -s1 * lc.inv_var;                           // :99
  gy = -s2 * lc.inv_var;                           // :100
}

template <int IMG, typename DT>
__global__ void __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(1)))
peaks_k1_tiledr(PeaksArgs a) {
  using TL = TiledR<IMG, 28, DT>;
  extern __shared__ double lds[];
  const DT* simg = k1_stage_image<TL>(lds, k1_image<DT>(a));
  const Consts& c = a.c;
  const K1Chain<TL::LPC> kc(a.n);
  if (kc.none) return;
  const int64_t ch = kc.chain, chr = kc.row;
  const bool writer = kc.writer;

  const double lnB = log_pos(c.B);
  const double sum_B = k1_background_V<TL>(simg, c.B, lnB);
  const LeanConsts lc = lean_consts(c);
  typename TL::Cache cache;
  TL::init(cache);
  double f = a.q[3 * chr], x = a.q[3 * chr + 1], y = a.q[3 * chr + 2];
  double vwin, gf, gx, gy;
  peaks_pass<TL>(lds, simg, cache, f, x, y, c, lc, lnB, vwin, gf, gx, gy);
  double V_prev = sum_B + vwin;                    // :195
  double V_last = V_prev;
  unsigned st = 0u;                                // 0: still descending
  int steps = 0;
  for (int i = 0; i < a.n_step; ++i) {
    const bool act = st == 0u;
    if (__builtin_amdgcn_ballot_w64(act) == 0) break;
    double nf = f, nx = x, ny = y;
    unsigned s1 = peaks_update(nf, nx, ny, gf, gx, gy, a.dt_f_coeff, a.dt_xy_coeff, a.f_lim);
    // a state that turned non-finite never passes a test (:209, :215): the
    // reference runs it to the cap, the kernel stops evaluating it here
    const bool bad = s1 == 0u && !(isfinite(nf) && isfinite(nx) && isfinite(ny));
    if (bad) s1 = RHMC_PEAK_CAP;
    f = act ? nf : f;                              // finished seeds keep their state
    x = act ? nx : x;
    y = act ? ny : y;
    steps = act ? (bad ? a.n_step : i + 1) : steps;
    double ngf, ngx, ngy;
    // (a stopped non-finite seed is evaluated at a fixed in-image point, so
    // that it does not make the wave re-read its windows every step)
    const bool fin = isfinite(f) && isfinite(x) && isfinite(y);
    peaks_pass<TL>(lds, simg, cache, fin ? f : 1.0, fin ? x : 0.0, fin ? y : 0.0, c, lc, lnB,
                   vwin, ngf, ngx, ngy);
    const double V_cur = sum_B + vwin;             // :213
    const bool go = act && s1 == 0u;               // V_cur is this step's V
    if (go && peaks_converged(V_cur, V_prev, a.rel_tol)) s1 = RHMC_PEAK_CONVERGED;
    V_last = go ? V_cur : V_last;
    V_prev = go ? V_cur : V_prev;                  // :218
    gf = go ? ngf : gf;
    gx = go ? ngx : gx;
    gy = go ? ngy : gy;
    st = act ? s1 : st;
  }
  if (st == 0u) {                                  // the for's else (:197)
    st = RHMC_PEAK_CAP;
    steps = a.n_step;
  }
  if (writer) {
    if (!(isfinite(f) && isfinite(x) && isfinite(y))) st |= RHMC_STATUS_NONFINITE;
    a.q[3 * ch] = f;
    a.q[3 * ch + 1] = x;
    a.q[3 * ch + 2] = y;
    if (a.steps) a.steps[ch] = steps;
    if (a.status) a.status[ch] = (int32_t)st;
    if (a.V) a.V[ch] = V_last;
  }
}

// ---- the stepwise path ------------------------------------------------------

struct PeaksStepArgs {
  double* q;              // [n][3] current state
  const double* grad;     // [n][3] dVdq at q (rhmc_gradient kind 0)
  double* q_new;          // [n][3] the updated state whose V the next launch evaluates
  const double* V_new;    // [n] V at q_new of the previous update (phase 1)
  double* V_prev;         // [n]
  double* V_last;         // [n]
  int32_t* steps;         // [n]
  int32_t* status;        // [n] 0 while descending
  int32_t* n_active;      // [1] seeds still descending (counted in phase 1)
  int64_t n;
  double f_lim, dt_f_coeff, dt_xy_coeff, rel_tol;
  int n_step, step;       // step: index i of the step this launch belongs to
};

// phase 0 (after the gradient at q): q_new = the update of q, FAINT / the
// non-finite stop decided, the step counted.  phase 1 (after V at q_new): the
// convergence test, V_prev, and q = q_new for the seeds that made the step.
// A finished seed (status != 0) is left alone; its q_new stays its q, so the
// batch launches between the phases evaluate it harmlessly.
template <int PHASE>
__global__ void __launch_bounds__(256) peaks_update_kernel(PeaksStepArgs a) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= a.n) return;
  unsigned st = (unsigned)a.status[i];
  if constexpr (PHASE == 0) {
    if (st != 0u) return;
    double f = a.q[3 * i], x = a.q[3 * i + 1], y = a.q[3 * i + 2];
    st = peaks_update(f, x, y, a.grad[3 * i], a.grad[3 * i + 1], a.grad[3 * i + 2],
                      a.dt_f_coeff, a.dt_xy_coeff, a.f_lim);
    const bool bad = st == 0u && !(isfinite(f) && isfinite(x) && isfinite(y));
    if (bad) st = RHMC_PEAK_CAP;
    a.steps[i] = bad ? a.n_step : a.step + 1;
    a.q_new[3 * i] = f;
    a.q_new[3 * i + 1] = x;
    a.q_new[3 * i + 2] = y;
    if (st != 0u) {                                // stopped: the state keeps the update
      a.q[3 * i] = f;
      a.q[3 * i + 1] = x;
      a.q[3 * i + 2] = y;
      a.status[i] = (int32_t)st;
    }
  } else {
    if (st != 0u) return;
    const double V_cur = a.V_new[i];
    if (peaks_converged(V_cur, a.V_prev[i], a.rel_tol)) st = RHMC_PEAK_CONVERGED;
    else if (a.step + 1 == a.n_step) st = RHMC_PEAK_CAP;
    a.V_last[i] = V_cur;
    a.V_prev[i] = V_cur;
    a.q[3 * i] = a.q_new[3 * i];
    a.q[3 * i + 1] = a.q_new[3 * i + 1];
    a.q[3 * i + 2] = a.q_new[3 * i + 2];
    a.status[i] = (int32_t)st;
    if (st == 0u) atomicAdd(a.n_active, 1);
  }
}

// Start of the stepwise path: V_prev = V_last = V(q) (already in V_prev),
// steps = 0, status = 0 (n_step == 0: CAP at once), q_new = q.
__global__ void __launch_bounds__(256) peaks_begin_kernel(PeaksStepArgs a) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= a.n) return;
  a.V_last[i] = a.V_prev[i];
  a.steps[i] = 0;
  a.status[i] = a.n_step == 0 ? (int32_t)RHMC_PEAK_CAP : 0;
  for (int k = 0; k < 3; ++k) a.q_new[3 * i + k] = a.q[3 * i + k];
}

// End: the non-finite flag and the caller's (nullable) outputs.
__global__ void __launch_bounds__(256)
peaks_end_kernel(PeaksStepArgs a, int32_t* steps_out, int32_t* status_out, double* V_out) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= a.n) return;
  unsigned st = (unsigned)a.status[i];
  int steps = a.steps[i];
  if (st == 0u) {                                  // the host loop ended at n_step
    st = RHMC_PEAK_CAP;
    steps = a.n_step;
  }
  if (!(isfinite(a.q[3 * i]) && isfinite(a.q[3 * i + 1]) && isfinite(a.q[3 * i + 2])))
    st |= RHMC_STATUS_NONFINITE;
  if (steps_out) steps_out[i] = steps;
  if (status_out) status_out[i] = (int32_t)st;
  if (V_out) V_out[i] = a.V_last[i];
}

}  // namespace rhmc
