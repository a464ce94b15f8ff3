// librhmc_post.so: the C-ABI of include/rhmc_post.h.  Argument checks, the
// grow-only workspace, the pass loop with the host-side lag search.
#include "rhmc_post.h"

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>
#include <new>
#include <string>
#include <vector>

#include "post_kernels.hpp"
#include "post_neff.hpp"

namespace {

thread_local std::string g_err;

int fail(int code, const std::string& msg) {
  g_err = msg;
  return code;
}

#define POST_HIP(call)                                                            \
  do {                                                                            \
    hipError_t e_ = (call);                                                       \
    if (e_ != hipSuccess)                                                         \
      return fail(RHMC_POST_ERR_HIP, std::string(#call ": ") + hipGetErrorString(e_)); \
  } while (0)

}  // namespace

struct rhmc_post_ctx {
  int device = 0;
  int32_t t_blk = 16;
  int32_t block = 256;
  double* d_work = nullptr;   // grow-only hipMalloc workspace
  size_t work_bytes = 0;
  double* h_pin = nullptr;    // grow-only pinned staging buffer
  size_t pin_bytes = 0;
};

namespace {

using rhmc_post::PassArgs;

// The calling thread's device for the length of a call.
struct DeviceGuard {
  int prev = -1;
  bool changed = false;
  hipError_t set(int device) {
    hipError_t e = hipGetDevice(&prev);
    if (e != hipSuccess) return e;
    if (prev == device) return hipSuccess;
    changed = true;
    return hipSetDevice(device);
  }
  ~DeviceGuard() {
    if (changed) (void)hipSetDevice(prev);
  }
};

struct Shape {
  int64_t n;       // length of a split sequence
  int64_t m;       // sequences
  int64_t extent;  // doubles from the base pointer to the last element read, + 1
};

// Shapes and strides first, pointers by the caller after this.
int check_layout(const rhmc_post_layout* L, int64_t warm_up, int64_t thin, Shape* out) {
  if (!L) return fail(RHMC_POST_ERR_ARG, "layout is NULL");
  if (L->n_chains < 2) return fail(RHMC_POST_ERR_ARG, "n_chains must be at least 2");
  if (L->D < 1) return fail(RHMC_POST_ERR_ARG, "D must be at least 1");
  if (L->n_iter < 1) return fail(RHMC_POST_ERR_ARG, "n_iter must be at least 1");
  if (thin < 1) return fail(RHMC_POST_ERR_ARG, "thin must be at least 1");
  if (warm_up < 0) return fail(RHMC_POST_ERR_ARG, "warm_up must not be negative");
  if (L->ld_iter < 0 || L->ld_chain < 0)
    return fail(RHMC_POST_ERR_ARG, "negative stride (ld_iter, ld_chain)");
  if (L->n_chains > (int64_t(1) << 40) || L->D > (int64_t(1) << 20) ||
      L->n_iter > (int64_t(1) << 40))
    return fail(RHMC_POST_ERR_ARG, "shape out of range");
  const int64_t kept = warm_up < L->n_iter ? (L->n_iter - warm_up + thin - 1) / thin : 0;
  const int64_t n = kept / 2;
  if (n < 3)
    return fail(RHMC_POST_ERR_ARG, "n = " + std::to_string(n) +
                                       " samples per split sequence; at least 3 are needed");
  out->n = n;
  out->m = 2 * L->n_chains;
  out->extent = (warm_up + (2 * n - 1) * thin) * L->ld_iter + (L->n_chains - 1) * L->ld_chain +
                L->D;
  return RHMC_POST_OK;
}

int ensure_work(rhmc_post_ctx* ctx, size_t bytes) {
  if (bytes <= ctx->work_bytes) return RHMC_POST_OK;
  if (ctx->d_work) {
    POST_HIP(hipFree(ctx->d_work));
    ctx->d_work = nullptr;
    ctx->work_bytes = 0;
  }
  if (hipMalloc(reinterpret_cast<void**>(&ctx->d_work), bytes) != hipSuccess) {
    ctx->d_work = nullptr;
    (void)hipGetLastError();
    return fail(RHMC_POST_ERR_NOMEM, "workspace of " + std::to_string(bytes) + " bytes");
  }
  ctx->work_bytes = bytes;
  return RHMC_POST_OK;
}

int ensure_pin(rhmc_post_ctx* ctx, size_t bytes) {
  if (bytes <= ctx->pin_bytes) return RHMC_POST_OK;
  if (ctx->h_pin) {
    POST_HIP(hipHostFree(ctx->h_pin));
    ctx->h_pin = nullptr;
    ctx->pin_bytes = 0;
  }
  if (hipHostMalloc(reinterpret_cast<void**>(&ctx->h_pin), bytes, hipHostMallocDefault) !=
      hipSuccess) {
    ctx->h_pin = nullptr;
    (void)hipGetLastError();
    return fail(RHMC_POST_ERR_NOMEM, "pinned buffer of " + std::to_string(bytes) + " bytes");
  }
  ctx->pin_bytes = bytes;
  return RHMC_POST_OK;
}

// The workspace of one call, in doubles.
struct Plan {
  int32_t T, B, S;
  int64_t gx;        // workgroups per half
  size_t off_mean, off_sd, off_partial, off_res, total;
};

int make_plan(const rhmc_post_ctx* ctx, const rhmc_post_layout& L, Plan* P) {
  P->T = ctx->t_blk;
  P->B = ctx->block;
  P->S = int32_t(std::min<int64_t>(L.D, P->B));
  const int64_t n_col = L.n_chains * L.D;
  P->gx = (n_col + P->B - 1) / P->B;
  if (P->gx > 0x7fffffffLL) return fail(RHMC_POST_ERR_ARG, "n_chains * D too large for one grid");
  const size_t md = size_t(2) * size_t(n_col);
  P->off_mean = 0;
  P->off_sd = md;
  P->off_partial = 2 * md;
  P->off_res = P->off_partial + size_t(2) * size_t(P->gx) * size_t(P->T) * size_t(P->S);
  P->total = P->off_res + size_t(3 + P->T) * size_t(L.D);
  return RHMC_POST_OK;
}

template <int T, bool FIRST>
void launch_pass_tb(const PassArgs& A, const Plan& P, hipStream_t st) {
  hipLaunchKernelGGL((rhmc_post::post_pass_kernel<T, FIRST>), dim3(unsigned(P.gx), 2), dim3(P.B),
                     0, st, A);
}

template <bool FIRST>
void launch_pass(const PassArgs& A, const Plan& P, hipStream_t st) {
  switch (P.T) {
    case 8: launch_pass_tb<8, FIRST>(A, P, st); break;
    default: launch_pass_tb<16, FIRST>(A, P, st); break;
  }
}

// One pass over the data for lags lag0 .. lag0 + T - 1 and the fixed-order
// sums of it: res[3 D ..] = sum of squared differences [T][D]; the first
// pass (first = true, lag0 = 1) also fills the moments res[0 .. 3 D).
int run_pass(rhmc_post_ctx* ctx, const double* d_x, const rhmc_post_layout& L, int64_t warm_up,
             int64_t thin, const Shape& sh, const Plan& P, int64_t lag0, bool first,
             hipStream_t st) {
  double* w = ctx->d_work;
  PassArgs A;
  A.x = d_x;
  A.ld_iter = L.ld_iter;
  A.ld_chain = L.ld_chain;
  A.n_chains = L.n_chains;
  A.D = L.D;
  A.warm = warm_up;
  A.thin = thin;
  A.n = sh.n;
  A.lag0 = lag0;
  A.col_mean = w + P.off_mean;
  A.col_sd = w + P.off_sd;
  A.partial = w + P.off_partial;
  A.S = P.S;
  if (first) launch_pass<true>(A, P, st); else launch_pass<false>(A, P, st);
  POST_HIP(hipGetLastError());
  double* res = w + P.off_res;
  if (first) {
    hipLaunchKernelGGL(rhmc_post::post_moment_reduce, dim3(unsigned(L.D)), dim3(64), 0, st,
                       A.col_mean, A.col_sd, sh.m, L.D, res);
    POST_HIP(hipGetLastError());
  }
  hipLaunchKernelGGL(rhmc_post::post_vario_reduce, dim3(unsigned(L.D), unsigned(P.T)), dim3(64),
                     0, st, A.partial, L.n_chains, L.D, P.B, P.S, P.T, P.gx, res + 3 * L.D);
  POST_HIP(hipGetLastError());
  const size_t from = first ? 0 : size_t(3) * L.D;
  const size_t cnt = size_t(3 + P.T) * L.D - from;
  POST_HIP(hipMemcpyAsync(ctx->h_pin + from, res + from, cnt * sizeof(double),
                          hipMemcpyDeviceToHost, st));
  POST_HIP(hipStreamSynchronize(st));
  return RHMC_POST_OK;
}

int prepare(rhmc_post_ctx* ctx, const rhmc_post_layout& L, Plan* P) {
  int rc = make_plan(ctx, L, P);
  if (rc) return rc;
  if ((rc = ensure_work(ctx, P->total * sizeof(double)))) return rc;
  return ensure_pin(ctx, size_t(3 + P->T) * size_t(L.D) * sizeof(double));
}

int convergence_device(rhmc_post_ctx* ctx, const double* d_x, const rhmc_post_layout& L,
                       int64_t warm_up, int64_t thin, int64_t max_lag, const Shape& sh,
                       double* R, double* n_eff, rhmc_post_detail* detail, hipStream_t st) {
  Plan P;
  int rc = prepare(ctx, L, &P);
  if (rc) return rc;
  const int64_t D = L.D, n = sh.n, m = sh.m;
  const int64_t lag_end = max_lag > 0 ? std::min<int64_t>(max_lag, n - 1) : n - 1;
  const double nan = std::numeric_limits<double>::quiet_NaN();

  if ((rc = run_pass(ctx, d_x, L, warm_up, thin, sh, P, 1, true, st))) return rc;
  int32_t passes = 1;
  const double* hp = ctx->h_pin;
  std::vector<double> var(D), W(D), Bv(D);
  std::vector<std::vector<double>> V(D);   // V[d][t - 1], grown per pass
  std::vector<char> done(D, 0);
  std::vector<int64_t> lags(D, 0);
  for (int64_t d = 0; d < D; ++d) {
    W[d] = hp[d] / double(m);
    Bv[d] = hp[2 * D + d] * double(n) / double(m - 1);
    var[d] = W[d] * double(n - 1) / double(n) + Bv[d] / double(n);
    if (std::isfinite(var[d]) && var[d] > 0.) {
      R[d] = std::sqrt(var[d] / W[d]);
    } else {
      R[d] = nan;
      n_eff[d] = nan;
      done[d] = 1;
    }
  }
  int64_t have = 0;   // lags computed so far
  for (;;) {
    const int64_t got = std::min<int64_t>(have + P.T, lag_end);
    bool all = true;
    for (int64_t d = 0; d < D; ++d) {
      if (done[d]) continue;
      for (int64_t t = have + 1; t <= got; ++t)
        V[d].push_back(hp[3 * D + (t - have - 1) * D + d] / double(m * (n - t)));
      const rhmc_post::NeffResult r = rhmc_post::neff_rule(m, n, var[d], V[d].data(), got);
      n_eff[d] = r.n_eff;
      lags[d] = r.lags;
      if (r.decided || got == lag_end) done[d] = 1; else all = false;
    }
    have = got;
    if (all) break;
    if ((rc = run_pass(ctx, d_x, L, warm_up, thin, sh, P, have + 1, false, st))) return rc;
    ++passes;
  }

  if (detail) {
    detail->d_split_mean = ctx->d_work + P.off_mean;
    detail->d_split_sd = ctx->d_work + P.off_sd;
    const size_t md = size_t(m) * size_t(D) * sizeof(double);
    if (detail->split_mean)
      POST_HIP(hipMemcpyAsync(detail->split_mean, detail->d_split_mean, md,
                              hipMemcpyDeviceToHost, st));
    if (detail->split_sd)
      POST_HIP(hipMemcpyAsync(detail->split_sd, detail->d_split_sd, md, hipMemcpyDeviceToHost,
                              st));
    if (detail->split_mean || detail->split_sd) POST_HIP(hipStreamSynchronize(st));
    for (int64_t d = 0; d < D; ++d) {
      if (detail->W) detail->W[d] = W[d];
      if (detail->B) detail->B[d] = Bv[d];
      if (detail->var) detail->var[d] = var[d];
      if (detail->lags_used) detail->lags_used[d] = int32_t(lags[d]);
    }
    detail->passes = passes;
    detail->n = int32_t(n);
  }
  return RHMC_POST_OK;
}

int check_accept(int64_t n_iter, int64_t n_chains, int64_t ld_iter, int64_t* start,
                 int64_t* end) {
  if (n_iter < 1) return fail(RHMC_POST_ERR_ARG, "n_iter must be at least 1");
  if (n_chains < 1) return fail(RHMC_POST_ERR_ARG, "n_chains must be at least 1");
  if (ld_iter < 0) return fail(RHMC_POST_ERR_ARG, "negative stride (ld_iter)");
  if (*start == -1 && *end == -1) {
    *start = 0;
    *end = n_iter;
  } else if (!(0 <= *start && *start < *end && *end <= n_iter)) {
    return fail(RHMC_POST_ERR_ARG,
                "start, end must be -1, -1 (the whole run) or 0 <= start < end <= n_iter");
  }
  return RHMC_POST_OK;
}

int launch_accept(const int32_t* d_accept, int64_t n_chains, int64_t ld_iter, int64_t start,
                  int64_t end, double* d_rate, hipStream_t st) {
  const int64_t g = (n_chains + 255) / 256;
  if (g > 0x7fffffffLL) return fail(RHMC_POST_ERR_ARG, "n_chains too large for one grid");
  hipLaunchKernelGGL(rhmc_post::post_accept_kernel, dim3(unsigned(g)), dim3(256), 0, st, d_accept,
                     n_chains, ld_iter, start, end, d_rate);
  POST_HIP(hipGetLastError());
  return RHMC_POST_OK;
}

// No C++ exception crosses the ABI.
template <class F>
int guarded(F&& f) {
  try {
    return f();
  } catch (const std::bad_alloc&) {
    return fail(RHMC_POST_ERR_NOMEM, "host allocation failed");
  } catch (const std::exception& e) {
    return fail(RHMC_POST_ERR_ARG, e.what());
  } catch (...) {
    return fail(RHMC_POST_ERR_ARG, "unknown exception");
  }
}

}  // namespace

extern "C" {

int rhmc_post_abi_version(void) { return RHMC_POST_ABI_VERSION; }

const char* rhmc_post_last_error(void) { return g_err.c_str(); }

int rhmc_post_create(int device, rhmc_post_ctx** out) {
  return guarded([&]() -> int {
    if (!out) return fail(RHMC_POST_ERR_ARG, "out is NULL");
    *out = nullptr;
    if (device < 0) return fail(RHMC_POST_ERR_ARG, "device must not be negative");
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n < 1) {
      (void)hipGetLastError();
      return fail(RHMC_POST_ERR_HIP, "no GPU visible");
    }
    if (device >= n) return fail(RHMC_POST_ERR_ARG, "no such device");
    rhmc_post_ctx* c = new rhmc_post_ctx;
    c->device = device;
    *out = c;
    return RHMC_POST_OK;
  });
}

void rhmc_post_destroy(rhmc_post_ctx* ctx) {
  if (!ctx) return;
  if (ctx->d_work || ctx->h_pin) {
    DeviceGuard g;
    (void)g.set(ctx->device);
    if (ctx->d_work) (void)hipFree(ctx->d_work);
    if (ctx->h_pin) (void)hipHostFree(ctx->h_pin);
  }
  delete ctx;
}

int rhmc_post_set_option(rhmc_post_ctx* ctx, int32_t option, int32_t value) {
  return guarded([&]() -> int {
    if (option == RHMC_POST_OPT_TBLK) {
      if (value != 8 && value != 16)
        return fail(RHMC_POST_ERR_ARG, "RHMC_POST_OPT_TBLK takes 8 or 16");
      if (!ctx) return fail(RHMC_POST_ERR_ARG, "ctx is NULL");
      ctx->t_blk = value;
      return RHMC_POST_OK;
    }
    if (option == RHMC_POST_OPT_BLOCK) {
      if (value != 64 && value != 128 && value != 256)
        return fail(RHMC_POST_ERR_ARG, "RHMC_POST_OPT_BLOCK takes 64, 128 or 256");
      if (!ctx) return fail(RHMC_POST_ERR_ARG, "ctx is NULL");
      ctx->block = value;
      return RHMC_POST_OK;
    }
    return fail(RHMC_POST_ERR_ARG, "unknown option");
  });
}

int rhmc_post_convergence_device(rhmc_post_ctx* ctx, const double* d_x,
                                 const rhmc_post_layout* layout, int64_t warm_up, int64_t thin,
                                 int64_t max_lag, double* R, double* n_eff,
                                 rhmc_post_detail* detail, void* stream) {
  return guarded([&]() -> int {
    Shape sh;
    int rc = check_layout(layout, warm_up, thin, &sh);
    if (rc) return rc;
    if (max_lag < 0) return fail(RHMC_POST_ERR_ARG, "max_lag must not be negative");
    if (!ctx || !d_x || !R || !n_eff)
      return fail(RHMC_POST_ERR_ARG, "NULL pointer (ctx, d_x, R or n_eff)");
    DeviceGuard g;
    POST_HIP(g.set(ctx->device));
    return convergence_device(ctx, d_x, *layout, warm_up, thin, max_lag, sh, R, n_eff, detail,
                              static_cast<hipStream_t>(stream));
  });
}

int rhmc_post_convergence(rhmc_post_ctx* ctx, const double* x, const rhmc_post_layout* layout,
                          int64_t warm_up, int64_t thin, int64_t max_lag, double* R,
                          double* n_eff, rhmc_post_detail* detail) {
  return guarded([&]() -> int {
    Shape sh;
    int rc = check_layout(layout, warm_up, thin, &sh);
    if (rc) return rc;
    if (max_lag < 0) return fail(RHMC_POST_ERR_ARG, "max_lag must not be negative");
    if (!ctx || !x || !R || !n_eff)
      return fail(RHMC_POST_ERR_ARG, "NULL pointer (ctx, x, R or n_eff)");
    DeviceGuard g;
    POST_HIP(g.set(ctx->device));
    double* d_x = nullptr;
    const size_t bytes = size_t(sh.extent) * sizeof(double);
    if (hipMalloc(reinterpret_cast<void**>(&d_x), bytes) != hipSuccess) {
      (void)hipGetLastError();
      return fail(RHMC_POST_ERR_NOMEM, "upload buffer of " + std::to_string(bytes) + " bytes");
    }
    hipError_t e = hipMemcpy(d_x, x, bytes, hipMemcpyHostToDevice);
    if (e != hipSuccess) {
      (void)hipFree(d_x);
      return fail(RHMC_POST_ERR_HIP, std::string("upload: ") + hipGetErrorString(e));
    }
    rc = convergence_device(ctx, d_x, *layout, warm_up, thin, max_lag, sh, R, n_eff, detail,
                            nullptr);
    (void)hipFree(d_x);
    return rc;
  });
}

int rhmc_post_variogram_device(rhmc_post_ctx* ctx, const double* d_x,
                               const rhmc_post_layout* layout, int64_t warm_up, int64_t thin,
                               int64_t lag0, int64_t n_lags, double* V, void* stream) {
  return guarded([&]() -> int {
    Shape sh;
    int rc = check_layout(layout, warm_up, thin, &sh);
    if (rc) return rc;
    if (lag0 < 1 || n_lags < 1 || lag0 > sh.n - 1 || n_lags > sh.n - lag0)
      return fail(RHMC_POST_ERR_ARG, "lags must lie in 1 .. n - 1");
    if (!ctx || !d_x || !V) return fail(RHMC_POST_ERR_ARG, "NULL pointer (ctx, d_x or V)");
    DeviceGuard g;
    POST_HIP(g.set(ctx->device));
    Plan P;
    if ((rc = prepare(ctx, *layout, &P))) return rc;
    const int64_t D = layout->D;
    for (int64_t done = 0; done < n_lags; done += P.T) {
      const int64_t first_lag = lag0 + done;
      if ((rc = run_pass(ctx, d_x, *layout, warm_up, thin, sh, P, first_lag, false,
                         static_cast<hipStream_t>(stream))))
        return rc;
      const int64_t cnt = std::min<int64_t>(P.T, n_lags - done);
      for (int64_t u = 0; u < cnt; ++u)
        for (int64_t d = 0; d < D; ++d)
          V[(done + u) * D + d] =
              ctx->h_pin[3 * D + u * D + d] / double(sh.m * (sh.n - (first_lag + u)));
    }
    return RHMC_POST_OK;
  });
}

int rhmc_post_neff(int64_t m, int64_t n, double var, const double* V, int64_t n_lags,
                   double* n_eff, int32_t* decided) {
  return guarded([&]() -> int {
    if (m < 2) return fail(RHMC_POST_ERR_ARG, "m must be at least 2");
    if (n < 3) return fail(RHMC_POST_ERR_ARG, "n must be at least 3");
    if (n_lags < 0) return fail(RHMC_POST_ERR_ARG, "n_lags must not be negative");
    if (!n_eff || !decided || (n_lags > 0 && !V))
      return fail(RHMC_POST_ERR_ARG, "NULL pointer (V, n_eff or decided)");
    const rhmc_post::NeffResult r =
        rhmc_post::neff_rule(m, n, var, V, std::min<int64_t>(n_lags, n - 1));
    *n_eff = r.n_eff;
    *decided = r.decided;
    return RHMC_POST_OK;
  });
}

int rhmc_post_acceptance_device(rhmc_post_ctx* ctx, const int32_t* d_accept, int64_t n_iter,
                                int64_t n_chains, int64_t ld_iter, int64_t start, int64_t end,
                                double* d_rate, void* stream) {
  return guarded([&]() -> int {
    int rc = check_accept(n_iter, n_chains, ld_iter, &start, &end);
    if (rc) return rc;
    if (!ctx || !d_accept || !d_rate)
      return fail(RHMC_POST_ERR_ARG, "NULL pointer (ctx, d_accept or d_rate)");
    DeviceGuard g;
    POST_HIP(g.set(ctx->device));
    return launch_accept(d_accept, n_chains, ld_iter, start, end, d_rate,
                         static_cast<hipStream_t>(stream));
  });
}

int rhmc_post_acceptance_fetch(rhmc_post_ctx* ctx, const int32_t* d_accept, int64_t n_iter,
                               int64_t n_chains, int64_t ld_iter, int64_t start, int64_t end,
                               double* rate, void* stream) {
  return guarded([&]() -> int {
    int rc = check_accept(n_iter, n_chains, ld_iter, &start, &end);
    if (rc) return rc;
    if (!ctx || !d_accept || !rate)
      return fail(RHMC_POST_ERR_ARG, "NULL pointer (ctx, d_accept or rate)");
    DeviceGuard g;
    POST_HIP(g.set(ctx->device));
    hipStream_t st = static_cast<hipStream_t>(stream);
    const size_t bytes = size_t(n_chains) * sizeof(double);
    if ((rc = ensure_work(ctx, bytes))) return rc;
    if ((rc = launch_accept(d_accept, n_chains, ld_iter, start, end, ctx->d_work, st))) return rc;
    POST_HIP(hipMemcpyAsync(rate, ctx->d_work, bytes, hipMemcpyDeviceToHost, st));
    POST_HIP(hipStreamSynchronize(st));
    return RHMC_POST_OK;
  });
}

int rhmc_post_acceptance(rhmc_post_ctx* ctx, const int32_t* accept, int64_t n_iter,
                         int64_t n_chains, int64_t ld_iter, int64_t start, int64_t end,
                         double* rate) {
  return guarded([&]() -> int {
    int rc = check_accept(n_iter, n_chains, ld_iter, &start, &end);
    if (rc) return rc;
    if (!ctx || !accept || !rate)
      return fail(RHMC_POST_ERR_ARG, "NULL pointer (ctx, accept or rate)");
    DeviceGuard g;
    POST_HIP(g.set(ctx->device));
    const size_t a_bytes = (size_t(n_iter - 1) * size_t(ld_iter) + size_t(n_chains)) *
                           sizeof(int32_t);
    const size_t r_bytes = size_t(n_chains) * sizeof(double);
    char* d = nullptr;
    const size_t r_off = (a_bytes + 7) / 8 * 8;
    if (hipMalloc(reinterpret_cast<void**>(&d), r_off + r_bytes) != hipSuccess) {
      (void)hipGetLastError();
      return fail(RHMC_POST_ERR_NOMEM, "upload buffer");
    }
    hipError_t e = hipMemcpy(d, accept, a_bytes, hipMemcpyHostToDevice);
    if (e == hipSuccess) {
      rc = launch_accept(reinterpret_cast<const int32_t*>(d), n_chains, ld_iter, start, end,
                         reinterpret_cast<double*>(d + r_off), nullptr);
      if (rc == RHMC_POST_OK) e = hipMemcpy(rate, d + r_off, r_bytes, hipMemcpyDeviceToHost);
    }
    (void)hipFree(d);
    if (rc) return rc;
    if (e != hipSuccess) return fail(RHMC_POST_ERR_HIP, std::string("copy: ") + hipGetErrorString(e));
    return RHMC_POST_OK;
  });
}

}  // extern "C"
