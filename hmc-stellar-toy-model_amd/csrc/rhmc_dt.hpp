// rhmc_dt.hpp — the trial of samplers.lightsource_gym.HMC_find_best_dt's
// step-size search (samplers.py:332-371, identical at :399-438) on the GPU:
// n_iter Metropolis iterations of explicit leapfrog on ONE star against a
// background image M (the residual of all the other stars), per task t
//
//   q = q0
//   for i in 0 .. n_iter-1:
//     p  = z[t][i]            (flux_only[t]: p[1] = p[2] = 0)        (:343-345)
//     E0 = V(q) + (p.p)/2     V = -sum(D ln L - L), L = M + f PSF    (:121-127)
//     ph = p - dt G(q)/2                                             (:352)
//     steps[t][i] times: q += dt ph ; ph -= dt G(q)                  (:354-356)
//     p  = ph + dt G(q)/2 ; dE = V(q) + (p.p)/2 - E0
//     accept = dE < 0 or lnu[t][i] < -dE, else q = the iteration's start (:366)
//
// G is dVdq_single's flux gradient -sum (D/L - 1) PSF broadcast over the three
// coordinates (RHMC_DT_GRAD_REFERENCE: what the reference's call computes,
// :77, :102-104) or the true (gf, gx, gy) (RHMC_DT_GRAD_FULL, :93-101).
//
// dt_trials_kernel<LANES, PPL>: one task per workgroup of LANES lanes; a
// workgroup walks tasks blockIdx.x, blockIdx.x + gridDim.x, ...  The image is
// always the whole image: M is a Poisson realisation minus f0 PSF and not
// bounded below, so no window argument holds, and no address depends on the
// state (q turns NaN or 1e300 in ordinary searches).  PPL > 0: each lane keeps
// PPL pixels of D and M in registers for the whole trial (pixel lane + LANES k),
// the R + C separable PSF factors of a gradient are written to LDS by the
// first lanes.  PPL == 0: the same body reading D and M from global memory
// and keeping the factors in a global table of the workgroup's own (any side).
//
// Every barrier is reached by every lane: the trip counts (tasks, n_iter,
// steps) are workgroup-uniform and no lane leaves early.  Sums run in a fixed
// order (lane-local in pixel order, the wave by wave_sum_dpp, the waves in
// index order), so a task's result depends on nothing but its own inputs.
// Non-finite values propagate (0 * NaN stays NaN) and end in a rejection.
#pragma once
#include "rhmc_exp.hpp"
#include "rhmc_mh.hpp"
#include "rhmc_wave.hpp"

namespace rhmc {

struct DtArgs {
  const double* D;            // [side][side] the context's image
  const double* bg;           // [n_bg][side][side]
  const int32_t* bg_index;    // [n]
  const double* q0;           // [n][3]
  const double* dt;           // [n][3]
  const int32_t* flux_only;   // nullable [n]
  const double* z;            // [n][n_iter][3], or all three NULL: Philox
  const int32_t* steps;       // [n][n_iter]
  const double* lnu;          // [n][n_iter]
  const uint64_t* stream_id;  // [n] (Philox)
  int32_t* n_accept;          // nullable [n]
  double* r_dE;               // the record, all nullable: [n][n_iter]
  int32_t* r_accept;          // [n][n_iter]
  double* r_q;                // [n][n_iter][3]
  double* r_z;                // [n][n_iter][3]
  int32_t* r_steps;           // [n][n_iter]
  double* r_lnu;              // [n][n_iter]
  double2* gtab;              // PPL == 0: [gridDim.x][2 side + 1] factor tables
  int64_t n;
  unsigned long long seed;
  int n_iter, grad, steps_min, steps_max, side, n_bg;
  double inv_two_sig2, inv_norm, inv_var;
};

constexpr unsigned kDtStepsDraw = 0x80000001u;  // Philox block index of the step count

// ln L for the V pass: log_pos where it holds (finite, normal, positive), the
// general log otherwise (0 -> -inf, negative -> NaN, like NumPy's).
__device__ __forceinline__ double dt_log(double lam) {
  double r = log_pos(lam);
  if (!(lam >= 0x1p-1000 && lam <= 0x1p1000)) r = log(lam);
  return r;
}

// One pixel of the gradient pass: rt = (f psf_i, f psf_i dx_i) of its row, ct =
// (psf_j, psf_j dy_j) of its column.
__device__ __forceinline__ void dt_grad_px(double d, double m, double2 rt, double2 ct,
                                           double& a0, double& a1, double& a2) {
  const double lam = fma(rt.x, ct.x, m);           // L = M + f PSF (:85)
  const double s = fma(d, rcp_nr(lam), -1.0);      // D/L - 1 (:88)
  const double sc = s * ct.x;
  a0 = fma(sc, rt.x, a0);
  a1 = fma(sc, rt.y, a1);
  a2 = fma(s * rt.x, ct.y, a2);
}
__device__ __forceinline__ double dt_v_px(double d, double m, double2 rt, double2 ct) {
  const double lam = fma(rt.x, ct.x, m);
  return fma(d, dt_log(lam), -lam);                // D ln L - L (:127)
}

template <int LANES, int PPL>
struct DtBlock {
  static constexpr int NW = LANES / kWave;
  static constexpr bool REG = PPL > 0;

  const DtArgs& a;
  double* s_exp;              // exp_neg's table
  double (*s_red)[NW][4];     // [2][NW][4] partial sums of the waves, two buffers
  double2* tab;               // [2 side + 1]: rows, columns, one zero entry
  int par = 0;
  // register-resident pixels: value of D, of M, (row entry | column entry << 16)
  double pd[REG ? PPL : 1], pm[REG ? PPL : 1];
  unsigned pidx[REG ? PPL : 1];
  const double* gD = nullptr;  // PPL == 0
  const double* gM = nullptr;

  __device__ DtBlock(const DtArgs& a_, double* e, double (*r)[NW][4], double2* t)
      : a(a_), s_exp(e), s_red(r), tab(t) {}

  __device__ void load_task(const double* M) {
    const int side = a.side, npix = side * side;
    if constexpr (REG) {
#pragma unroll
      for (int k = 0; k < PPL; ++k) {
        const int p = (int)threadIdx.x + LANES * k;
        const bool in = p < npix;
        const int pc = in ? p : 0;
        const int i = pc / side, j = pc - i * side;
        pd[k] = in ? a.D[pc] : 0.0;                // an absent pixel: D = 0, M = 1 and the
        pm[k] = in ? M[pc] : 1.0;                  // zero entry: adds exactly 0 to every sum
        pidx[k] = in ? ((unsigned)i | ((unsigned)(side + j) << 16))
                     : ((unsigned)(2 * side) | ((unsigned)(2 * side) << 16));
      }
    } else {
      gD = a.D;
      gM = M;
    }
  }

  // The separable factors at (f, x, y) into the table; ends with a barrier.
  __device__ void factors(double f, double x, double y) {
    const int side = a.side;
    const double fs = flux_fold(f) * a.inv_norm;
    for (int t = threadIdx.x; t < 2 * side; t += LANES) {
      const bool row = t < side;
      const double d = ((double)(row ? t : t - side) + 0.5) - (row ? x : y);
      double e = exp_neg(-(d * d) * a.inv_two_sig2, s_exp);
      e = row ? e * fs : e;
      tab[t] = double2{e, e * d};
    }
    __syncthreads();
  }

  // Sum of up to three values over the workgroup, the same bits in every lane.
  __device__ void block_sum(double& v0, double& v1, double& v2) {
    v0 = wave_sum_dpp(v0);
    v1 = wave_sum_dpp(v1);
    v2 = wave_sum_dpp(v2);
    if constexpr (NW > 1) {
      const int w = threadIdx.x / kWave;
      if (lane_id() == 0) {
        s_red[par][w][0] = v0;
        s_red[par][w][1] = v1;
        s_red[par][w][2] = v2;
      }
      __syncthreads();
      v0 = s_red[par][0][0];
      v1 = s_red[par][0][1];
      v2 = s_red[par][0][2];
#pragma unroll
      for (int k = 1; k < NW; ++k) {
        v0 += s_red[par][k][0];
        v1 += s_red[par][k][1];
        v2 += s_red[par][k][2];
      }
      par ^= 1;
    } else {
      __syncthreads();   // the table's readers are done before its next writer
    }
  }

  // G(q) (:93-104); the factors of q end up in the table.
  __device__ void gradient(double f, double x, double y, double& g0, double& g1, double& g2) {
    factors(f, x, y);
    double a0 = 0.0, a1 = 0.0, a2 = 0.0;
    if constexpr (REG) {
#pragma unroll
      for (int k = 0; k < PPL; ++k)
        dt_grad_px(pd[k], pm[k], tab[pidx[k] & 0xffffu], tab[pidx[k] >> 16], a0, a1, a2);
    } else {
      const int side = a.side, npix = side * side;
      for (int p = threadIdx.x; p < npix; p += LANES) {
        const int i = p / side, j = p - i * side;
        dt_grad_px(gD[p], gM[p], tab[i], tab[side + j], a0, a1, a2);
      }
    }
    block_sum(a0, a1, a2);
    const double gf = -a0 / flux_fold(f);          // :94
    if (a.grad == RHMC_DT_GRAD_FULL) {
      g0 = gf;
      g1 = -a1 * a.inv_var;                        // :99
      g2 = -a2 * a.inv_var;                        // :100
    } else {
      g0 = g1 = g2 = gf;                           // f_only=True, broadcast (:352)
    }
  }

  // V at the state whose factors the table holds (:121-127).
  __device__ double potential() {
    double v = 0.0, u1 = 0.0, u2 = 0.0;
    if constexpr (REG) {
#pragma unroll
      for (int k = 0; k < PPL; ++k) {
        const double t = dt_v_px(pd[k], pm[k], tab[pidx[k] & 0xffffu], tab[pidx[k] >> 16]);
        v += ((int)threadIdx.x + LANES * k < a.side * a.side) ? t : 0.0;
      }
    } else {
      const int side = a.side, npix = side * side;
      for (int p = threadIdx.x; p < npix; p += LANES) {
        const int i = p / side, j = p - i * side;
        v += dt_v_px(gD[p], gM[p], tab[i], tab[side + j]);
      }
    }
    block_sum(v, u1, u2);
    return -v;
  }

  __device__ void trial(int64_t t) {
    const int n_iter = a.n_iter;
    int bi = a.bg_index[t];                        // (the host entry point rejects these)
    bi = bi < 0 ? 0 : (bi >= a.n_bg ? a.n_bg - 1 : bi);
    load_task(a.bg + (int64_t)bi * a.side * a.side);
    double q0 = a.q0[3 * t], q1 = a.q0[3 * t + 1], q2 = a.q0[3 * t + 2];
    const double d0 = a.dt[3 * t], d1 = a.dt[3 * t + 1], d2 = a.dt[3 * t + 2];
    const bool fo = a.flux_only && a.flux_only[t] != 0;
    const long long sid = a.z ? 0 : (long long)a.stream_id[t];
    const bool writer = threadIdx.x == 0;
    double Vq = 0.0;
    int n_acc = 0;
    // Iteration -1 is the warm-up that evaluates V(q0): no draws, no steps, no
    // decision.  It shares the loop body so that the pixel passes are
    // instantiated once (registers).
    for (int it = -1; it < n_iter; ++it) {
      const bool warm = it < 0;
      const int64_t r = t * n_iter + (warm ? 0 : it);
      double z0 = 0.0, z1 = 0.0, z2 = 0.0, lnu = 0.0;
      int ns = 0;
      if (warm) {
      } else if (a.z) {
        z0 = a.z[3 * r];
        z1 = a.z[3 * r + 1];
        z2 = a.z[3 * r + 2];
        ns = a.steps[r];
        ns = ns < 0 ? 0 : (ns > 65535 ? 65535 : ns);
        lnu = a.lnu[r];
      } else {
        z0 = philox_normal(a.seed, sid, it, 0);
        z1 = philox_normal(a.seed, sid, it, 1);
        z2 = philox_normal(a.seed, sid, it, 2);
        const U4 b = philox_block(a.seed, sid, it, kDtStepsDraw);
        const unsigned range = (unsigned)(a.steps_max - a.steps_min);
        ns = a.steps_min + (int)(((unsigned long long)b.x * range) >> 32);
        lnu = log(philox_uniform(a.seed, sid, it));
      }
      ns = __builtin_amdgcn_readfirstlane(ns);     // workgroup-uniform by construction
      double p0 = z0, p1 = fo ? 0.0 : z1, p2 = fo ? 0.0 : z2;   // :343-345
      const double E0 = Vq + ((p0 * p0 + p1 * p1) + p2 * p2) / 2.0;   // :348
      double g0, g1, g2, h0 = p0, h1 = p1, h2 = p2;
      double n0 = q0, n1 = q1, n2 = q2;
      for (int s = 0; s <= ns; ++s) {
        if (s > 0) {                               // :355
          n0 = n0 + d0 * h0;
          n1 = n1 + d1 * h1;
          n2 = n2 + d2 * h2;
        }
        gradient(n0, n1, n2, g0, g1, g2);
        if (s > 0) {                               // :356
          h0 = h0 - d0 * g0;
          h1 = h1 - d1 * g1;
          h2 = h2 - d2 * g2;
        } else {                                   // :352, the first half step
          h0 = p0 - d0 * g0 / 2.0;
          h1 = p1 - d1 * g1 / 2.0;
          h2 = p2 - d2 * g2 / 2.0;
        }
      }
      p0 = h0 + d0 * g0 / 2.0;                     // :357, G at the same state
      p1 = h1 + d1 * g1 / 2.0;
      p2 = h2 + d2 * g2 / 2.0;
      const double Vn = potential();               // the table holds (n0, n1, n2)
      if (warm) {
        Vq = Vn;
        continue;
      }
      const double dE = (Vn + ((p0 * p0 + p1 * p1) + p2 * p2) / 2.0) - E0;   // :360-363
      const bool acc = (dE < 0.0) || (lnu < -dE);  // :366 (NaN: false)
      if (acc) {
        q0 = n0;
        q1 = n1;
        q2 = n2;
        Vq = Vn;
        ++n_acc;
      }
      if (writer) {
        if (a.r_dE) a.r_dE[r] = dE;
        if (a.r_accept) a.r_accept[r] = acc ? 1 : 0;
        if (a.r_q) {
          a.r_q[3 * r] = q0;
          a.r_q[3 * r + 1] = q1;
          a.r_q[3 * r + 2] = q2;
        }
        if (a.r_z) {
          a.r_z[3 * r] = z0;
          a.r_z[3 * r + 1] = z1;
          a.r_z[3 * r + 2] = z2;
        }
        if (a.r_steps) a.r_steps[r] = ns;
        if (a.r_lnu) a.r_lnu[r] = lnu;
      }
    }
    if (writer && a.n_accept) a.n_accept[t] = n_acc;
  }
};

template <int LANES, int PPL>
__global__ void __launch_bounds__(LANES) dt_trials_kernel(DtArgs a) {
  constexpr int NW = LANES / kWave;
  __shared__ double s_exp[kExpTab];
  __shared__ double s_red[2][NW][4];
  extern __shared__ double2 s_dt_tab[];            // PPL > 0: [2 side + 1]
  double2* tab;
  if constexpr (PPL > 0) tab = s_dt_tab;
  else tab = a.gtab + (int64_t)blockIdx.x * (2 * a.side + 1);
  exp_tab_fill(s_exp);
  if (threadIdx.x == 0) tab[2 * a.side] = double2{0.0, 0.0};
  __syncthreads();
  DtBlock<LANES, PPL> b(a, s_exp, s_red, tab);
  for (int64_t t = blockIdx.x; t < a.n; t += gridDim.x) b.trial(t);
}

}  // namespace rhmc
