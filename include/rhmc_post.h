/*
 * rhmc_post.h — C-ABI of librhmc_post.so: MCMC post-processing of recorded
 * chains on the GPU (Gelman-Rubin R-hat, effective sample size, acceptance
 * rates), for the records the engine leaves in device memory
 * (rhmc_mh_record, include/rhmc.h).
 *
 * Reference interface (file:line into the reference checkout):
 *   rhmc_post_convergence(_device)   utils.convergence_stats (utils.py:86-168)
 *   rhmc_post_variogram_device       utils.variogram (utils.py:170-188) on the
 *                                    split sequences of convergence_stats
 *   rhmc_post_neff                   the lag search of convergence_stats
 *                                    (utils.py:141-166) on given variograms
 *   rhmc_post_acceptance(_device)    utils.acceptance_rate (utils.py:192-209)
 * rhmc_amd/diagnostics.py restates those in NumPy and is the specification.
 *
 * The library is separate from the engine: it needs no rhmc_ctx and does not
 * link librhmc.so.  It takes raw device pointers and a stream, so it serves
 * the engine's records, torch tensors and the reversible-jump driver's padded
 * rows alike.
 *
 * Semantics (quirks of the reference included).  Per chain: drop warm_up
 * rows, keep every thin-th row, trim to even length 2n, split into halves:
 * m = 2 n_chains sequences of length n; sequence 2c + h is half h of chain c.
 *   W   = mean over sequences of the standard deviations (ddof = 1), not of
 *         the variances
 *   B   = n / (m - 1) * sum_s (mean_s - mean_all)^2
 *   var = W (n - 1) / n + B / n,   R = sqrt(var / W)
 *   V_t = sum_s sum_j (y_s[j + t] - y_s[j])^2 / (m (n - t)),  1 <= t <= n - 1
 *   rho_t = 1 - V_t / (2 var)
 *   rho_1 < 0.05: sum = 0.  Else lags are added until, at odd t,
 *   rho_{t+1} + rho_{t+2} < 0 (sum = rho_1 + ... + rho_t), or until t = n - 2;
 *   a negative sum becomes 0;  n_eff = m n / (1 + 2 sum).
 * Deviations: max_lag > 0 caps the search (max_lag = 0: the reference's
 * unbounded one); a coordinate whose pooled var is 0 or not finite gets NaN R
 * and NaN n_eff without a lag search (the reference ends at NaN there too,
 * after exhausting every lag); acceptance takes start = end = -1 (the whole
 * run) or 0 <= start < end <= n_iter, not the reference's negative indices.
 *
 * Conventions
 *   - Every call returns 0 or a negative RHMC_POST_ERR_* code;
 *     rhmc_post_last_error() gives a thread-local message.  No C++ exception
 *     crosses the ABI.
 *   - Arguments are checked before any HIP call: shapes and strides first,
 *     pointers after them.
 *   - `stream` is a hipStream_t passed as void* (NULL = the null stream).
 *   - One context must not be used by two threads at once.
 *   - Results are pinned: sums across chains run in a fixed order (no
 *     floating-point atomics), so two identical calls agree bit for bit.
 */
#ifndef RHMC_POST_H
#define RHMC_POST_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define RHMC_POST_ABI_VERSION 1

enum {
  RHMC_POST_OK = 0,
  RHMC_POST_ERR_ARG = -1,    /* bad argument (shape, stride, NULL ...) */
  RHMC_POST_ERR_HIP = -2,    /* a HIP runtime call failed               */
  RHMC_POST_ERR_NOMEM = -3   /* device or pinned allocation failed      */
};

/*
 * Where the samples are: x[it][c][d] = base[it * ld_iter + c * ld_chain + d],
 * strides in doubles, coordinate stride 1.  The engine's record
 * [n_iter][n_chains][D] is {ld_iter = n_chains * D, ld_chain = D}; the
 * reference's [Nchain][Niter][D] is {ld_iter = D, ld_chain = Niter * D}; rows
 * padded beyond D (the RJ driver's [n][3 N_max]) have ld_chain > D.  Reads are
 * coalesced when ld_chain is the small stride.
 */
typedef struct rhmc_post_layout {
  int64_t n_iter;
  int64_t n_chains;
  int64_t D;
  int64_t ld_iter;
  int64_t ld_chain;
} rhmc_post_layout;

/*
 * Optional extras of rhmc_post_convergence(_device).  The caller zeroes the
 * struct and sets the host pointers it wants filled (each nullable).
 * d_split_mean / d_split_sd are set by the call: device arrays
 * [2 n_chains][D] of the split sequences' means and standard deviations in
 * the context's workspace, valid until the next call on the context.
 */
typedef struct rhmc_post_detail {
  const double* d_split_mean; /* out: device [2 n_chains][D]                 */
  const double* d_split_sd;   /* out: device [2 n_chains][D]                 */
  double* split_mean;         /* in: host [2 n_chains][D] or NULL            */
  double* split_sd;           /* in: host [2 n_chains][D] or NULL            */
  double* W;                  /* in: host [D] or NULL                        */
  double* B;                  /* in: host [D] or NULL                        */
  double* var;                /* in: host [D] or NULL                        */
  int32_t* lags_used;         /* in: host [D] or NULL: variograms the search
                                 read (the reference loop's count; 0 for a
                                 coordinate without a search, the cap when
                                 max_lag stopped it)                         */
  int32_t passes;             /* out: passes made over the data              */
  int32_t n;                  /* out: length of a split sequence             */
} rhmc_post_detail;

typedef struct rhmc_post_ctx rhmc_post_ctx;

/* Context options.  Results do not depend on RHMC_POST_OPT_TBLK; the block
 * size changes the order of the sums across chains (last bits). */
enum {
  RHMC_POST_OPT_TBLK = 1,   /* lags per pass: 8 or 16 (default)              */
  RHMC_POST_OPT_BLOCK = 2   /* threads per workgroup: 64, 128 or 256 (default) */
};
int rhmc_post_set_option(rhmc_post_ctx* ctx, int32_t option, int32_t value);

/* ABI version of the loaded library (== RHMC_POST_ABI_VERSION when in sync). */
int rhmc_post_abi_version(void);
/* Thread-local message of the last failing call ("" if none). */
const char* rhmc_post_last_error(void);

/* A context on `device`.  It owns a grow-only hipMalloc workspace and a
 * pinned staging buffer, released by rhmc_post_destroy. */
int rhmc_post_create(int device, rhmc_post_ctx** out);
void rhmc_post_destroy(rhmc_post_ctx* ctx);

/*
 * R-hat and n_eff of every coordinate of the fp64 device array d_x.  R,
 * n_eff: host [D], filled when the call returns (the call synchronises
 * `stream`: the lag search is decided on the host after each pass).  The
 * first pass over the data computes the moments and the first block of lags,
 * each later pass one more block, until every coordinate is decided.
 * Errors: n_chains < 2, D < 1, thin < 1, warm_up < 0, max_lag < 0, n < 3, a
 * negative stride, a NULL pointer.
 */
int rhmc_post_convergence_device(rhmc_post_ctx* ctx, const double* d_x,
                                 const rhmc_post_layout* layout, int64_t warm_up, int64_t thin,
                                 int64_t max_lag, double* R, double* n_eff,
                                 rhmc_post_detail* detail, void* stream);
/* The same with a host x: uploads, runs and frees. */
int rhmc_post_convergence(rhmc_post_ctx* ctx, const double* x, const rhmc_post_layout* layout,
                          int64_t warm_up, int64_t thin, int64_t max_lag, double* R,
                          double* n_eff, rhmc_post_detail* detail);

/* V_t of the split sequences for t = lag0 .. lag0 + n_lags - 1
 * (1 <= lag0, lag0 + n_lags - 1 <= n - 1) into the host array
 * V[n_lags][D]; synchronises `stream`. */
int rhmc_post_variogram_device(rhmc_post_ctx* ctx, const double* d_x,
                               const rhmc_post_layout* layout, int64_t warm_up, int64_t thin,
                               int64_t lag0, int64_t n_lags, double* V, void* stream);

/*
 * The stopping rule on given variograms (host only, no HIP call): m sequences
 * of length n, pooled variance var, V[i] = V_{i+1} for i < n_lags.  *decided
 * = 1 when the rule fired (or ran to t = n - 2, or var is 0 or not finite:
 * NaN) within the lags given, and *n_eff is final; *decided = 0 when it
 * needs more lags, and *n_eff is the value from the lags so far (what a
 * max_lag cap reports).
 */
int rhmc_post_neff(int64_t m, int64_t n, double var, const double* V, int64_t n_lags,
                   double* n_eff, int32_t* decided);

/* d_rate[c] = sum of d_accept[it][c] over start <= it < end, over
 * (end - start); d_accept int32 [n_iter][n_chains] with row stride ld_iter
 * (in int32s).  start = end = -1: the whole run.  Asynchronous on `stream`. */
int rhmc_post_acceptance_device(rhmc_post_ctx* ctx, const int32_t* d_accept, int64_t n_iter,
                                int64_t n_chains, int64_t ld_iter, int64_t start, int64_t end,
                                double* d_rate, void* stream);
/* The same with the rates into the host array rate[n_chains], through the
 * context's workspace; synchronises `stream`. */
int rhmc_post_acceptance_fetch(rhmc_post_ctx* ctx, const int32_t* d_accept, int64_t n_iter,
                               int64_t n_chains, int64_t ld_iter, int64_t start, int64_t end,
                               double* rate, void* stream);
/* The same with host accept and rate: uploads, runs, downloads and frees. */
int rhmc_post_acceptance(rhmc_post_ctx* ctx, const int32_t* accept, int64_t n_iter,
                         int64_t n_chains, int64_t ld_iter, int64_t start, int64_t end,
                         double* rate);

#ifdef __cplusplus
}
#endif

#endif /* RHMC_POST_H */
