// Device code of librhmc_post.so (gfx950, wave64, fp64 throughout).
//
// One lane owns one (split sequence, coordinate) column and walks its n kept
// samples in time; consecutive lanes own consecutive (chain, coordinate)
// pairs of one half, so that a row of the iteration-major record is read
// coalesced.  A pass computes T lags lag0 .. lag0 + T - 1: the lead sample
// y[i] meets the T samples y[i - lag0 - u], u < T, which sit in a register
// ring with static indices (the time loop is unrolled by T).  The first pass
// (lag0 = 1) feeds the ring from the lead sample itself and runs Welford's
// moments on it, so it reads every kept sample once; a later pass reads a
// second, delayed stream lag0 - 1 rows behind the lead.
//
// Sums across chains are store-and-sum: a workgroup folds its lanes' sums by
// coordinate in LDS in a fixed order and stores the partials; a second
// kernel adds the partials in a fixed order.  No floating-point atomics.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace rhmc_post {

struct PassArgs {
  const double* x;
  int64_t ld_iter, ld_chain;
  int64_t n_chains, D;
  int64_t warm, thin;
  int64_t n;          // length of a split sequence
  int64_t lag0;       // first lag of the pass
  double* col_mean;   // [2 n_chains][D]  (first pass)
  double* col_sd;     // [2 n_chains][D]  (first pass)
  double* partial;    // [2 gridDim.x][T][S], S = min(D, blockDim.x)
  int32_t S;
};

// One group of T samples, k = k0 .. k0 + T - 1 (k = i - (lag0 - 1)): the lead
// a = y[i] meets ring entries pushed u + 1 steps ago (lag lag0 + u, present
// once u < k), then e = y[k] enters the ring.  CHECK: the first group (ring
// filling) and the last one (k may pass n_tot); both tests are wave-uniform.
template <int T, bool FIRST, bool CHECK>
__device__ __forceinline__ void post_group(const double (&lead)[T], const double (&del)[T],
                                           double (&ring)[T], double (&acc)[T], int64_t k0,
                                           int64_t n_tot, double& mean, double& m2) {
#pragma unroll
  for (int r = 0; r < T; ++r) {
    const int64_t k = k0 + r;
    if (CHECK && k >= n_tot) break;
    const double a = lead[r];
#pragma unroll
    for (int u = 0; u < T; ++u) {
      const double dl = a - ring[(r - u - 1 + 2 * T) % T];
      // an explicit fma: a column's sums round the same in every variant
      if (!CHECK || u < k) acc[u] = __builtin_fma(dl, dl, acc[u]);
    }
    ring[r] = FIRST ? a : del[r];
    if (FIRST) {   // Welford: k samples seen before this one
      const double dm = a - mean;
      mean += dm / double(k + 1);
      m2 += dm * (a - mean);
    }
  }
}

template <int T, bool FIRST>
__device__ __forceinline__ void post_load(double (&lead)[T], double (&del)[T], const double* p,
                                          int64_t step, int64_t lag0, int64_t k0,
                                          int64_t n_tot) {
#pragma unroll
  for (int r = 0; r < T; ++r) {
    // past the end: the last sample again (a valid address, never used)
    const int64_t k = (k0 + r < n_tot) ? k0 + r : n_tot - 1;
    lead[r] = p[(k + lag0 - 1) * step];
    if (!FIRST) del[r] = p[k * step];
  }
}

template <int T, bool FIRST>
__global__ void __launch_bounds__(256) post_pass_kernel(PassArgs A) {
  __shared__ double sh[256];
  const int B = blockDim.x;
  const int tid = threadIdx.x;
  const int64_t n_col = A.n_chains * A.D;       // columns of one half
  const int64_t g0 = int64_t(blockIdx.x) * B;   // the workgroup's first column
  const int h = blockIdx.y;
  const bool active = g0 + tid < n_col;
  // an idle lane reads the last column and contributes nothing
  const int64_t j = active ? g0 + tid : n_col - 1;
  const int64_t c = j / A.D, d = j - c * A.D;
  const int64_t step = A.thin * A.ld_iter;
  const double* p = A.x + (A.warm + int64_t(h) * A.n * A.thin) * A.ld_iter + c * A.ld_chain + d;
  const int64_t n_tot = A.n - A.lag0 + 1;       // lead samples i = lag0 - 1 .. n - 1

  double ring[T], acc[T], cur[T], dcur[T], nxt[T];
#pragma unroll
  for (int u = 0; u < T; ++u) { ring[u] = 0.; acc[u] = 0.; dcur[u] = 0.; nxt[u] = 0.; }
  double mean = 0., m2 = 0.;

  // the first pass prefetches the next group while it works on this one; a
  // later pass holds two streams and loads each group as it comes (with the
  // prefetch its 16-lag form needs more than 256 registers)
  post_load<T, FIRST>(cur, dcur, p, step, A.lag0, 0, n_tot);
  for (int64_t k0 = 0; k0 < n_tot; k0 += T) {
    const bool more = k0 + T < n_tot;
    if (!FIRST && k0 > 0) post_load<T, FIRST>(cur, dcur, p, step, A.lag0, k0, n_tot);
    if (FIRST && more) post_load<T, FIRST>(nxt, dcur, p, step, A.lag0, k0 + T, n_tot);
    if (k0 == 0 || k0 + T > n_tot)
      post_group<T, FIRST, true>(cur, dcur, ring, acc, k0, n_tot, mean, m2);
    else
      post_group<T, FIRST, false>(cur, dcur, ring, acc, k0, n_tot, mean, m2);
    if (FIRST && more) {
#pragma unroll
      for (int r = 0; r < T; ++r) cur[r] = nxt[r];
    }
  }

  if (FIRST && active) {
    const int64_t s = 2 * c + h;
    A.col_mean[s * A.D + d] = mean;
    A.col_sd[s * A.D + d] = sqrt(m2 / double(A.n - 1));
  }

  // fold the lanes by coordinate: slot q takes lanes q, q + D, q + 2D, ...
  // (coordinate (g0 + q) % D), in that order
  const int64_t blk = int64_t(h) * gridDim.x + blockIdx.x;
#pragma unroll
  for (int u = 0; u < T; ++u) {
    sh[tid] = active ? acc[u] : 0.;
    __syncthreads();
    if (tid < A.S) {
      double s = sh[tid];
      for (int64_t l = tid + A.D; l < B; l += A.D) s += sh[l];
      A.partial[(blk * T + u) * A.S + tid] = s;
    }
    __syncthreads();
  }
}

// Fixed-order sum of a 64-lane workgroup's values (lane 0 holds it).
__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
  return v;
}

// out[u][d] = sum over both halves and every workgroup of the partials of
// coordinate d.  grid (D, T), 64 threads: lane l takes items l, l + 64, ...
// in order, then a shuffle tree.
__global__ void __launch_bounds__(64) post_vario_reduce(const double* partial, int64_t n_chains,
                                                        int64_t D, int32_t B, int32_t S,
                                                        int32_t T, int64_t gx, double* out) {
  const int64_t d = blockIdx.x;
  const int u = blockIdx.y;
  double s = 0.;
  if (D < B) {
    // every workgroup covers every coordinate: slot (d - g0) mod D
    for (int64_t b = threadIdx.x; b < 2 * gx; b += 64) {
      const int64_t bx = b < gx ? b : b - gx;
      const int64_t q = (d + D - (bx * B) % D) % D;
      s += partial[(b * T + u) * S + q];
    }
  } else {
    // S = B: one slot per lane; walk the chains
    for (int64_t i = threadIdx.x; i < 2 * n_chains; i += 64) {
      const int64_t h = i < n_chains ? 0 : 1;
      const int64_t j = (i - h * n_chains) * D + d;
      const int64_t bx = j / B;
      s += partial[((h * gx + bx) * T + u) * S + (j - bx * B)];
    }
  }
  s = wave_sum(s);
  if (threadIdx.x == 0) out[int64_t(u) * D + d] = s;
}

// Per coordinate: sum of the split standard deviations, mean of the split
// means, and the centred sum of squares of the split means around it (its own
// pass: B never comes from sum(mean^2) - sum(mean)^2 / m).  grid D, 64 threads.
// out[0][d] = sum sd, out[1][d] = mean_all, out[2][d] = sum (mean_s - mean_all)^2.
__global__ void __launch_bounds__(64) post_moment_reduce(const double* col_mean,
                                                         const double* col_sd, int64_t m,
                                                         int64_t D, double* out) {
  const int64_t d = blockIdx.x;
  double ssd = 0., sm = 0.;
  for (int64_t s = threadIdx.x; s < m; s += 64) {
    ssd += col_sd[s * D + d];
    sm += col_mean[s * D + d];
  }
  ssd = wave_sum(ssd);
  sm = wave_sum(sm);
  const double mean_all = __shfl(sm, 0, 64) / double(m);
  double sq = 0.;
  for (int64_t s = threadIdx.x; s < m; s += 64) {
    const double e = col_mean[s * D + d] - mean_all;
    sq += e * e;
  }
  sq = wave_sum(sq);
  if (threadIdx.x == 0) {
    out[d] = ssd;
    out[D + d] = mean_all;
    out[2 * D + d] = sq;
  }
}

// rate[c] = sum_{start <= it < end} accept[it][c] / (end - start); lane = chain.
__global__ void __launch_bounds__(256) post_accept_kernel(const int32_t* a, int64_t n_chains,
                                                          int64_t ld_iter, int64_t start,
                                                          int64_t end, double* rate) {
  const int64_t c = int64_t(blockIdx.x) * blockDim.x + threadIdx.x;
  if (c >= n_chains) return;
  int64_t s = 0;
  int64_t it = start;
  for (; it + 8 <= end; it += 8) {
    int32_t v[8];
#pragma unroll
    for (int r = 0; r < 8; ++r) v[r] = a[(it + r) * ld_iter + c];
#pragma unroll
    for (int r = 0; r < 8; ++r) s += v[r];
  }
  for (; it < end; ++it) s += a[it * ld_iter + c];
  rate[c] = double(s) / double(end - start);
}

}  // namespace rhmc_post
