// rhmc_chain.hpp — device side of the Metropolis-Hastings loop around the
// random-length trajectories of samplers.lightsource_gym.HMC_random
// (samplers.py:460-572) and RHMC_random_diag (:668-825): the momentum draw, E
// and the accept test, one thread per chain below 8 stars and one wave per
// chain (lanes over the 3K coordinates) from 8.  The trajectories and V reuse
// the existing kernels (launch_hmc_random_t, launch_energy).
//
// chain_turn_kernel, turn i = 0 .. n_iter, is "accept iteration i" fused with
// "draw and record iteration i + 1", so that an iteration is three launches
// (turn, trajectory, energy), all on one stream with no host round trip:
//   i == 0 : p = z[0] sqrt(M(q)); E_chain[0] = E(q, p); dE_chain[0] = 0 (:507-513, :725-731)
//   i >= 1 : E1 = E(q', p') with V(q') from the energy launch and M(q');
//            dE = E1 - E0; accept iff dE < 0 or lnu[i] < -dE (:563), then
//            q <- q' and V(q) <- V(q'), else q stays
//            q_chain[i] = q
//   i < n_iter : p = z[i+1] sqrt(M(q)); E0 = E(q, p) (V(q) is carried);
//            E_chain[i+1] = E0, dE_chain[i+1] = E0 - E0 of the turn before;
//            q' = q; the length of trajectory i + 1
// E (:1152-1161) is +inf when any flux is below f_lim, else V + K with
//   unit metric      K = sum(p^2)/2                                   (:1171)
//   diagonal metric  M = (1/f, f factor1, f factor1) per star (:574-590),
//                    K = (sum(p^2/M) + log|prod M|)/2, the product a running
//                    product in index order like np.prod              (:1173)
// NaN compares false everywhere: a NaN chain never accepts.
// Draws: the host's arrays, or Philox-4x32-10 (rhmc_mh.hpp) under `seed` with
// the counter (draw, iter0 + i, stream_id[chain]): normal j is philox_normal,
// the length kDtStepsDraw with rhmc_dt_trials' mapping, u block 0x80000000.
// A chain reads and writes its own rows only, so its result depends on
// nothing but its own start, seed, stream_id and iter0.
#pragma once
#include "rhmc_dt.hpp"
#include "rhmc_mh.hpp"
#include "rhmc_wave.hpp"

namespace rhmc {

struct ChainArgs {
  double* q;                  // [n][3K] current state (updated on accept)
  double* q_prop;             // [n][3K] proposal
  double* p;                  // [n][3K] momentum
  double* V_cur;              // [n] V of the current state
  double* V_prop;             // [n] V of the proposal (written by the energy kernel)
  double* E0;                 // [n] E at the iteration's start
  int32_t* steps;             // [n] the next trajectory's lengths (device draws)
  const double* z;            // [n_iter+1][n][3K], or all three NULL: Philox
  const int32_t* h_steps;     // [n_iter][n]
  const double* lnu;          // [n_iter][n]
  const uint64_t* stream_id;  // nullable [n] (Philox): the chain index
  double* q_chain;            // the record, all nullable: [n_iter+1][n][3K]
  double* E_chain;            // [n_iter+1][n]
  double* dE_chain;           // [n_iter+1][n]
  int32_t* accept;            // [n_iter][n]
  double* r_z;                // [n_iter+1][n][3K]
  int32_t* r_steps;           // [n_iter][n]
  double* r_lnu;              // [n_iter][n]
  int64_t n;
  unsigned long long seed;
  double factor1, f_lim;
  int K, iter, n_iter, iter0, steps_min, steps_max;
};

// E(q, p) of one chain from its V (:1152-1175).  DRAW: p = z[row] sqrt(M(q))
// is drawn, stored and recorded on the way; else p is read.  WAVE: the lanes of
// the chain's wave share the coordinates and every lane returns the same bits.
template <bool WAVE, bool DIAG, bool DRAW>
__device__ __forceinline__ double chain_energy(const ChainArgs& a, const double* q, double* p,
                                               double V, int64_t ch, long long sid, int row,
                                               int lane) {
  const int d = 3 * a.K;
  const int first = WAVE ? lane : 0, stride = WAVE ? kWave : 1;
  double t = 0.0;
  bool below = false;
  for (int idx = first; idx < d; idx += stride) {
    const int j = idx % 3;
    const double f = q[idx - j];
    below = below || (f < a.f_lim);                // :1157-1159
    double m = 1.0;
    if constexpr (DIAG) m = (j == 0) ? 1.0 / f : f * a.factor1;   // G(f), F(f) (:592-625)
    double pv;
    if constexpr (DRAW) {
      const int64_t zi = ((int64_t)row * a.n + ch) * d + idx;
      const double zz = a.z ? a.z[zi] : philox_normal(a.seed, sid, a.iter0 + row, idx);
      pv = DIAG ? zz * sqrt(m) : zz;               // p_sample() * np.sqrt(M) (:725, :746)
      p[idx] = pv;
      if (a.r_z) a.r_z[zi] = zz;
    } else {
      pv = p[idx];
    }
    if constexpr (DIAG) t += (pv * pv) / m;
    else t += pv * pv;
  }
  if constexpr (WAVE) {
    t = wave_sum(t);
    below = __any(below) != 0;
  }
  if constexpr (DIAG) {                            // np.prod(M): index order, every lane
    double prod = 1.0;
    for (int k = 0; k < a.K; ++k) {
      const double f = q[3 * k];
      const double fm = f * a.factor1;
      prod *= 1.0 / f;
      prod *= fm;
      prod *= fm;
    }
    t += log(fabs(prod));
  }
  const double E = V + t / 2.0;
  return below ? __builtin_inf() : E;
}

template <bool WAVE, bool DIAG>
__global__ void __launch_bounds__(256) chain_turn_kernel(ChainArgs a) {
  const int64_t ch = WAVE ? (int64_t)blockIdx.x * (blockDim.x / kWave) + threadIdx.x / kWave
                          : (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (ch >= a.n) return;                           // (a whole wave when WAVE)
  const int lane = WAVE ? lane_id() : 0;
  const bool lead = lane == 0;
  const int d = 3 * a.K;
  const int first = WAVE ? lane : 0, stride = WAVE ? kWave : 1;
  double* q = a.q + ch * d;
  double* qp = a.q_prop + ch * d;
  double* p = a.p + ch * d;
  const long long sid = a.z ? 0 : (a.stream_id ? (long long)a.stream_id[ch] : (long long)ch);
  const int i = a.iter;
  const int64_t r = (int64_t)i * a.n + ch;         // row i of this chain
  double V = a.V_cur[ch], E_prev;
  bool acc = false;
  if (i == 0) {                                    // E(q0, p_initial) (:507-513)
    E_prev = chain_energy<WAVE, DIAG, true>(a, q, p, V, ch, sid, 0, lane);
    if (lead) {
      if (a.E_chain) a.E_chain[r] = E_prev;
      if (a.dE_chain) a.dE_chain[r] = 0.0;
    }
  } else {                                         // the decision of iteration i
    const double V1 = a.V_prop[ch];
    const double E1 = chain_energy<WAVE, DIAG, false>(a, qp, p, V1, ch, sid, 0, lane);
    E_prev = a.E0[ch];
    const double dE = E1 - E_prev;                 // :560
    const int64_t ri = r - a.n;                    // row i - 1 of the [n_iter] records
    const double lnu = a.lnu ? a.lnu[ri] : log(philox_uniform(a.seed, sid, a.iter0 + i));
    acc = (dE < 0.0) || (lnu < -dE);               // :563 (NaN: false)
    if (acc) V = V1;
    if (lead) {
      if (acc) a.V_cur[ch] = V1;
      if (a.accept) a.accept[ri] = acc ? 1 : 0;
      if (a.r_lnu) a.r_lnu[ri] = lnu;
    }
  }
  const double* qc = acc ? qp : q;                 // the state after iteration i
  if (a.q_chain)
    for (int idx = first; idx < d; idx += stride) a.q_chain[r * d + idx] = qc[idx];
  if (i < a.n_iter) {                              // the start of iteration i + 1
    const double E0 = chain_energy<WAVE, DIAG, true>(a, qc, p, V, ch, sid, i + 1, lane);
    int ns;
    if (a.h_steps) {
      ns = a.h_steps[r];
    } else {
      const U4 b = philox_block(a.seed, sid, a.iter0 + i + 1, kDtStepsDraw);
      const unsigned range = (unsigned)(a.steps_max - a.steps_min);
      ns = a.steps_min + (int)(((unsigned long long)b.x * range) >> 32);
    }
    if (lead) {
      a.E0[ch] = E0;
      if (a.E_chain) a.E_chain[r + a.n] = E0;
      if (a.dE_chain) a.dE_chain[r + a.n] = E0 - E_prev;     // :526
      if (!a.h_steps) a.steps[ch] = ns;
      if (a.r_steps) a.r_steps[r] = ns;
    }
  }
  // after every read of q and q': q <- q' on accept, else q' <- q, the next
  // trajectory's start
  for (int idx = first; idx < d; idx += stride) {
    if (acc) q[idx] = qp[idx];
    else qp[idx] = q[idx];
  }
}

}  // namespace rhmc
