// rhmc_kernels.hip — the main translation unit of librhmc.so: the context,
// error reporting, option handling and the C-ABI declared in include/rhmc.h.
// The kernels live in the rhmc_*.hpp headers (the one-wave-per-chain ones, the
// slotted frame for the LDS-image, windowed and dense gradient policies and
// the LDS-image step, in rhmc_perwave.hpp); rhmc_select.hpp chooses the kernel family of a call and
// rhmc_launch.hpp builds its arguments and launches it.  Every kernel but the
// two of rhmc_dense_ilp.hip is instantiated, and so launched, from this unit.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <type_traits>
#include <memory>
#include <mutex>
#include <string>
#include <vector>

#include "rhmc.h"
#include "rhmc_select.hpp"
#include "rhmc_datagen.hpp"
#include "rhmc_mh.hpp"
#include "rhmc_tiledl.hpp"
#include "rhmc_tiledr.hpp"
#include "rhmc_tiledrk.hpp"
#include "rhmc_mhk1.hpp"
#include "rhmc_mhpk.hpp"
#include "rhmc_peaks.hpp"
#include "rhmc_dt.hpp"
#include "rhmc_chain.hpp"
#include "rhmc_pixk.hpp"
#include "rhmc_wave.hpp"
#include "rhmc_windowed.hpp"
#include "rhmc_dense.hpp"
#include "rhmc_rows.hpp"
#include "rhmc_perwave.hpp"
#include "rhmc_hess.hpp"

namespace rhmc {
// The dense kernel's one-slot leapfrog (K <= 64 on 32/48-px images: B4, the
// reference's big-sim4 run) is compiled in rhmc_dense_ilp.hip with the max-ILP
// scheduler; this translation unit only launches it.
extern template __global__ void leapfrog_win_kernel<DenseG<32>, 1>(LeapArgs);
extern template __global__ void leapfrog_win_kernel<DenseG<48>, 1>(LeapArgs);
}  // namespace rhmc

using namespace rhmc;

static thread_local std::string g_err;

static int fail(int code, const std::string& msg) {
  g_err = msg;
  return code;
}

#define HIP_TRY(expr)                                                               \
  do {                                                                              \
    hipError_t e_ = (expr);                                                         \
    if (e_ != hipSuccess)                                                           \
      return fail(RHMC_ERR_HIP, std::string(#expr) + ": " + hipGetErrorString(e_)); \
  } while (0)

struct rhmc_ctx {
  int device = 0;
  hipStream_t stream = nullptr;
  int rows = 0, cols = 0;
  double* d_D = nullptr;
  float* d_Df = nullptr;   // D in fp32, valid when img_f32
  int* d_flag = nullptr;
  bool img_f32 = false;    // every pixel of D is exactly representable in fp32
  // scratch for the host-pointer entry points
  void* scratch = nullptr;
  size_t scratch_bytes = 0;
  void* mh_scratch = nullptr;      // MH driver work arrays (q', p, V, V', E0)
  size_t mh_scratch_bytes = 0;
  int max_lds = 0;
  int n_cu = 0;
  int kernel = RHMC_KERNEL_AUTO;   // RHMC_OPT_KERNEL
  int mh_fused = 1;                // RHMC_OPT_MH_FUSED
  int window_split = 0;            // RHMC_OPT_WINDOW_SPLIT (0: by batch size)
  int peaks_fused = 1;             // RHMC_OPT_PEAKS_FUSED
  int32_t* h_pin = nullptr;        // pinned word: find_peaks' stepwise path polls through it
  int dt_lanes = 0;                // RHMC_OPT_DT_LANES
  void* dt_tab = nullptr;          // dt_trials' factor tables of the global-memory path
  size_t dt_tab_bytes = 0;
  int table_mode = RHMC_TABLES_STREAM;  // RHMC_OPT_TABLES
  // WinGG factor tables, one buffer per stream (work_tables).  A launch holds a
  // lease (shared_ptr) on its buffer from the lookup until the launch is
  // enqueued, so a concurrent grow on the same stream cannot free it early.
  struct TabBuf {
    void* p = nullptr;
    size_t bytes = 0;
    hipStream_t s = nullptr;
    bool synced = false;   // rhmc_ctx_destroy synchronised the device already
    ~TabBuf() {
      if (!p) return;
      if (!synced) (void)hipStreamSynchronize(s);  // the last launch reading it
      (void)hipFree(p);
    }
  };
  struct StreamTables {
    hipStream_t s;
    std::shared_ptr<TabBuf> buf;
  };
  mutable std::mutex tab_mu;
  mutable std::vector<StreamTables> tabs;
};

#include "rhmc_launch.hpp"

namespace {

int check_common(rhmc_ctx* ctx, int64_t n_chains, int32_t K) {
  if (!ctx) return fail(RHMC_ERR_ARG, "ctx is NULL");
  if (!ctx->d_D) return fail(RHMC_ERR_ARG, "no image uploaded");
  if (n_chains < 0) return fail(RHMC_ERR_ARG, "n_chains < 0");
  if (K < 1 || K > kMaxK) return fail(RHMC_ERR_ARG, "K must be in [1, 1024]");
  if (n_chains > ((int64_t)1 << 40)) return fail(RHMC_ERR_ARG, "n_chains too large");
  return RHMC_OK;
}

// The checks the two find_peaks entry points share (n == 0 after them: a
// no-op); the arguments first, so that they are checked without a device too.
int check_peaks(rhmc_ctx* ctx, const rhmc_params* P, const rhmc_peaks_opts* o, const double* q,
                int64_t n) {
  if (!P) return fail(RHMC_ERR_ARG, "params is NULL");
  if (!o) return fail(RHMC_ERR_ARG, "opts is NULL");
  if (n < 0) return fail(RHMC_ERR_ARG, "n < 0");
  if (n > ((int64_t)1 << 31)) return fail(RHMC_ERR_ARG, "n too large (2^31 seeds at most)");
  if (o->reserved != 0) return fail(RHMC_ERR_ARG, "opts.reserved must be 0");
  if (o->n_step < 0 || o->n_step > 1000000)
    return fail(RHMC_ERR_ARG, "opts.n_step must be in [0, 10^6]");
  if (!(std::isfinite(o->f_lim) && std::isfinite(o->dt_f_coeff) &&
        std::isfinite(o->dt_xy_coeff) && std::isfinite(o->rel_tol)))
    return fail(RHMC_ERR_ARG, "opts: non-finite coefficient");
  if (!q) return fail(RHMC_ERR_ARG, "q is NULL");
  if (!ctx) return fail(RHMC_ERR_ARG, "ctx is NULL");
  if (n > 0 && !ctx->d_D) return fail(RHMC_ERR_ARG, "no image uploaded");
  return RHMC_OK;
}

// The checks the two diag_random entry points share (n == 0 after them: a
// no-op), arguments before the context like check_peaks.  host_call: steps
// is readable, so every length and the trace's row count are checked (the
// kernels of the device entry point write no row past trace_rows).
int check_diag(rhmc_ctx* ctx, const rhmc_params* P, const rhmc_diag_opts* o, const double* q,
               const double* p, const int32_t* steps, int64_t n, int32_t K, const double* trace,
               bool host_call) {
  if (!P) return fail(RHMC_ERR_ARG, "params is NULL");
  if (!o) return fail(RHMC_ERR_ARG, "opts is NULL");
  if (n < 0) return fail(RHMC_ERR_ARG, "n_chains < 0");
  if (n > ((int64_t)1 << 40)) return fail(RHMC_ERR_ARG, "n_chains too large");
  if (K < 1 || K > kMaxK) return fail(RHMC_ERR_ARG, "K must be in [1, 1024]");
  if (o->reserved != 0) return fail(RHMC_ERR_ARG, "opts.reserved must be 0");
  if (!std::isfinite(o->dt)) return fail(RHMC_ERR_ARG, "opts.dt is not finite");
  if (!(std::isfinite(o->factor1) && o->factor1 > 0.0))
    return fail(RHMC_ERR_ARG, "opts.factor1 must be finite and > 0");
  if (!steps) return fail(RHMC_ERR_ARG, "steps is NULL");
  if (n > 0 && (!q || !p)) return fail(RHMC_ERR_ARG, "q/p is NULL");
  if (trace && o->trace_rows < 2)
    return fail(RHMC_ERR_ARG, "opts.trace_rows must exceed the longest trajectory (>= 2)");
  if (host_call) {
    int32_t longest = 0;
    for (int64_t i = 0; i < n; ++i) {
      if (steps[i] < 1) return fail(RHMC_ERR_ARG, "steps[i] must be >= 1");
      longest = steps[i] > longest ? steps[i] : longest;
    }
    if (trace && o->trace_rows <= longest)
      return fail(RHMC_ERR_ARG, "opts.trace_rows = " + std::to_string(o->trace_rows) +
                                    " must exceed the longest trajectory (" +
                                    std::to_string(longest) + " steps)");
  }
  if (!ctx) return fail(RHMC_ERR_ARG, "ctx is NULL");
  if (n > 0 && !ctx->d_D) return fail(RHMC_ERR_ARG, "no image uploaded");
  return RHMC_OK;
}

// The checks the hess_derivs / hess_random entry points share (n == 0 after
// them: a no-op), arguments before the context like check_peaks.  traj: the
// trajectory's arguments (opts, p, steps; f_lim >= 0, which the break test of
// hess_trajectory relies on); host_call: steps is readable.
int check_hess(rhmc_ctx* ctx, const rhmc_params* P, const rhmc_hess_opts* o, const double* q,
               const double* p, const int32_t* steps, int64_t n, int32_t K, bool traj,
               bool host_call) {
  if (!P) return fail(RHMC_ERR_ARG, "params is NULL");
  if (traj && !o) return fail(RHMC_ERR_ARG, "opts is NULL");
  if (n < 0) return fail(RHMC_ERR_ARG, "n_chains < 0");
  if (n > ((int64_t)1 << 40)) return fail(RHMC_ERR_ARG, "n_chains too large");
  if (K < 1 || K > kMaxK) return fail(RHMC_ERR_ARG, "K must be in [1, 1024]");
  if (traj) {
    if (o->reserved[0] != 0 || o->reserved[1] != 0)
      return fail(RHMC_ERR_ARG, "opts.reserved must be 0");
    if (!(std::isfinite(o->dt_f) && std::isfinite(o->dt_xy)))
      return fail(RHMC_ERR_ARG, "opts.dt_f / opts.dt_xy is not finite");
    if (!(P->f_lim >= 0.0))
      return fail(RHMC_ERR_ARG, "params.f_lim must be >= 0 for the Hessian-metric trajectory");
    if (!steps) return fail(RHMC_ERR_ARG, "steps is NULL");
    if (n > 0 && (!q || !p)) return fail(RHMC_ERR_ARG, "q/p is NULL");
    if (host_call)
      for (int64_t i = 0; i < n; ++i)
        if (steps[i] < 1) return fail(RHMC_ERR_ARG, "steps[i] must be >= 1");
  } else if (n > 0 && !q) {
    return fail(RHMC_ERR_ARG, "q is NULL");
  }
  if (!ctx) return fail(RHMC_ERR_ARG, "ctx is NULL");
  if (n > 0 && !ctx->d_D) return fail(RHMC_ERR_ARG, "no image uploaded");
  return RHMC_OK;
}

// The checks the two dt_trials entry points share (n == 0 after them: a
// no-op), arguments before the context like check_peaks.
int check_dt(rhmc_ctx* ctx, const rhmc_params* P, const rhmc_dt_opts* o, const double* bg,
             int32_t n_bg, const int32_t* bg_index, const double* q0, const double* dt, int64_t n,
             const double* z, const int32_t* steps, const double* lnu,
             const uint64_t* stream_id, bool host_call) {
  if (!P) return fail(RHMC_ERR_ARG, "params is NULL");
  if (!o) return fail(RHMC_ERR_ARG, "opts is NULL");
  if (n < 0) return fail(RHMC_ERR_ARG, "n < 0");
  if (n > ((int64_t)1 << 31)) return fail(RHMC_ERR_ARG, "n too large (2^31 tasks at most)");
  if (o->reserved[0] != 0 || o->reserved[1] != 0)
    return fail(RHMC_ERR_ARG, "opts.reserved must be 0");
  if (o->n_iter < 1 || o->n_iter > 1024)
    return fail(RHMC_ERR_ARG, "opts.n_iter must be in [1, 1024]");
  if (o->grad != RHMC_DT_GRAD_REFERENCE && o->grad != RHMC_DT_GRAD_FULL)
    return fail(RHMC_ERR_ARG, "opts.grad must be RHMC_DT_GRAD_REFERENCE or RHMC_DT_GRAD_FULL");
  const int n_draws = (z != nullptr) + (steps != nullptr) + (lnu != nullptr);
  if (n_draws != 0 && n_draws != 3)
    return fail(RHMC_ERR_ARG, "z, steps and lnu: pass all three or none");
  if (n_draws == 0) {
    if (!(o->steps_min >= 0 && o->steps_min < o->steps_max && o->steps_max <= 65536))
      return fail(RHMC_ERR_ARG, "opts: 0 <= steps_min < steps_max <= 65536 for device draws");
    if (!stream_id) return fail(RHMC_ERR_ARG, "stream_id is NULL (device draws)");
  }
  if (!bg) return fail(RHMC_ERR_ARG, "bg is NULL");
  if (n_bg < 1) return fail(RHMC_ERR_ARG, "n_bg < 1");
  if (!bg_index) return fail(RHMC_ERR_ARG, "bg_index is NULL");
  if (!q0) return fail(RHMC_ERR_ARG, "q0 is NULL");
  if (!dt) return fail(RHMC_ERR_ARG, "dt is NULL");
  if (host_call) {                                 // (the device entry point clamps these)
    for (int64_t t = 0; t < n; ++t)
      if (bg_index[t] < 0 || bg_index[t] >= n_bg)
        return fail(RHMC_ERR_ARG, "bg_index[" + std::to_string(t) + "] outside [0, n_bg)");
    if (steps)
      for (int64_t r = 0; r < n * o->n_iter; ++r)
        if (steps[r] < 0 || steps[r] > 65535)
          return fail(RHMC_ERR_ARG, "steps[" + std::to_string(r) + "] outside 0..65535");
  }
  if (!ctx) return fail(RHMC_ERR_ARG, "ctx is NULL");
  if (n > 0 && !ctx->d_D) return fail(RHMC_ERR_ARG, "no image uploaded");
  return RHMC_OK;
}

// The checks the two chain entry points share (n == 0 after them: a no-op),
// arguments before the context like check_peaks.  host_call: steps is readable.
int check_chain(rhmc_ctx* ctx, const rhmc_params* P, const rhmc_chain_opts* o, const double* dt,
                const double* q, int64_t n, int32_t K, const double* z, const int32_t* steps,
                const double* lnu, bool host_call) {
  if (!P) return fail(RHMC_ERR_ARG, "params is NULL");
  if (!o) return fail(RHMC_ERR_ARG, "opts is NULL");
  if (n < 0) return fail(RHMC_ERR_ARG, "n < 0");
  if (n > ((int64_t)1 << 31)) return fail(RHMC_ERR_ARG, "n too large (2^31 chains at most)");
  if (K < 1 || K > kMaxK) return fail(RHMC_ERR_ARG, "K must be in [1, 1024]");
  if (o->reserved != 0) return fail(RHMC_ERR_ARG, "opts.reserved must be 0");
  if (o->metric != RHMC_CHAIN_UNIT && o->metric != RHMC_CHAIN_DIAG)
    return fail(RHMC_ERR_ARG, "opts.metric must be RHMC_CHAIN_UNIT or RHMC_CHAIN_DIAG");
  if (o->n_iter < 0) return fail(RHMC_ERR_ARG, "opts.n_iter < 0");
  if (o->iter0 < 0) return fail(RHMC_ERR_ARG, "opts.iter0 < 0");
  if ((int64_t)o->iter0 + o->n_iter > 0x7fffffff)
    return fail(RHMC_ERR_ARG, "opts.iter0 + opts.n_iter exceeds 2^31 - 1");
  if (o->metric == RHMC_CHAIN_DIAG) {
    if (!std::isfinite(o->dt_global)) return fail(RHMC_ERR_ARG, "opts.dt_global is not finite");
    if (!(std::isfinite(o->factor1) && o->factor1 > 0.0))
      return fail(RHMC_ERR_ARG, "opts.factor1 must be finite and > 0");
  } else if (!dt) {
    return fail(RHMC_ERR_ARG, "dt is NULL (RHMC_CHAIN_UNIT)");
  }
  const int n_draws = (z != nullptr) + (steps != nullptr) + (lnu != nullptr);
  if (n_draws != 0 && n_draws != 3)
    return fail(RHMC_ERR_ARG, "z, steps and lnu: pass all three or none");
  if (n_draws == 0 &&
      !(o->steps_min >= 1 && o->steps_min < o->steps_max && o->steps_max <= 65536))
    return fail(RHMC_ERR_ARG, "opts: 1 <= steps_min < steps_max <= 65536 for device draws");
  if (n > 0 && !q) return fail(RHMC_ERR_ARG, "q is NULL");
  if (host_call && steps)
    for (int64_t r = 0; r < n * o->n_iter; ++r)
      if (steps[r] < 1) return fail(RHMC_ERR_ARG, "steps[" + std::to_string(r) + "] must be >= 1");
  if (!ctx) return fail(RHMC_ERR_ARG, "ctx is NULL");
  if (n > 0 && !ctx->d_D) return fail(RHMC_ERR_ARG, "no image uploaded");
  return RHMC_OK;
}

// Staging of the host-buffer entry points: the buffers of one call as parts
// of ctx->scratch, each aligned to 256 bytes.  add() lists a buffer, run()
// sizes the scratch, uploads the inputs, calls the launch, downloads the
// outputs and waits for the context's stream.  A NULL host pointer keeps its
// part on the device (optional outputs the kernel writes anyway) without a copy.
struct Staging {
  enum Dir { kDevice = 0, kIn = 1, kOut = 2, kInOut = 3 };
  struct Part {
    void* host;
    size_t off, bytes;
    int dir;
  };
  rhmc_ctx* ctx;
  Part part[16];
  int n = 0;
  size_t total = 0;

  explicit Staging(rhmc_ctx* c) : ctx(c) {}
  int add(const void* host, size_t bytes, int dir) {
    part[n] = {const_cast<void*>(host), total, bytes, host && bytes ? dir : (int)kDevice};
    total += (bytes + 255) & ~(size_t)255;
    return n++;
  }
  // The device side of part i (valid inside run()'s launch); NULL if empty.
  template <class T>
  T* dev(int i) const {
    return part[i].bytes ? (T*)((char*)ctx->scratch + part[i].off) : nullptr;
  }
  template <class Launch>
  int run(Launch&& launch) {
    if (int rc = ensure_scratch(ctx, total + 256)) return rc;
    for (int i = 0; i < n; ++i)
      if (part[i].dir & kIn)
        HIP_TRY(hipMemcpyAsync(dev<void>(i), part[i].host, part[i].bytes, hipMemcpyHostToDevice,
                               ctx->stream));
    if (int rc = launch()) return rc;
    for (int i = 0; i < n; ++i)
      if (part[i].dir & kOut)
        HIP_TRY(hipMemcpyAsync(part[i].host, dev<void>(i), part[i].bytes, hipMemcpyDeviceToHost,
                               ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    return RHMC_OK;
  }
};

// fp32 copy of the image and whether it is exact (every pixel == (float)pixel,
// NaN counts as inexact): the register-window kernel caches window pixels in
// fp32 when it is (rhmc_tiledr.hpp).
__global__ void image_f32_kernel(const double* __restrict__ D, float* __restrict__ Df,
                                 int64_t n, int* __restrict__ inexact) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n;
       i += (int64_t)gridDim.x * blockDim.x) {
    const double v = D[i];
    const float f = (float)v;
    Df[i] = f;
    if (!((double)f == v)) atomicOr(inexact, 1);
  }
}

// Called with the new image already enqueued on ctx->stream; synchronises.
int refresh_image_f32(rhmc_ctx* ctx) {
  const int64_t n = (int64_t)ctx->rows * ctx->cols;
  if (ctx->d_Df) HIP_TRY(hipFree(ctx->d_Df));
  ctx->d_Df = nullptr;
  ctx->img_f32 = false;
  if (hipMalloc(&ctx->d_Df, (size_t)n * sizeof(float)) != hipSuccess)
    return fail(RHMC_ERR_NOMEM, "hipMalloc fp32 image failed");
  if (!ctx->d_flag && hipMalloc(&ctx->d_flag, sizeof(int)) != hipSuccess)
    return fail(RHMC_ERR_NOMEM, "hipMalloc flag failed");
  HIP_TRY(hipMemsetAsync(ctx->d_flag, 0, sizeof(int), ctx->stream));
  const int blocks = (int)std::min<int64_t>((n + 255) / 256, 1024);
  hipLaunchKernelGGL(image_f32_kernel, dim3(blocks), dim3(256), 0, ctx->stream, ctx->d_D,
                     ctx->d_Df, n, ctx->d_flag);
  HIP_TRY(hipGetLastError());
  int inexact = 1;
  HIP_TRY(hipMemcpyAsync(&inexact, ctx->d_flag, sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
  HIP_TRY(hipStreamSynchronize(ctx->stream));
  ctx->img_f32 = inexact == 0;
  return RHMC_OK;
}

}  // namespace

extern "C" {

int rhmc_abi_version(void) { return RHMC_ABI_VERSION; }

const char* rhmc_last_error(void) { return g_err.c_str(); }

int rhmc_device_count(int* n) {
  if (!n) return fail(RHMC_ERR_ARG, "n is NULL");
  int c = 0;
  hipError_t e = hipGetDeviceCount(&c);
  *n = (e == hipSuccess) ? c : 0;
  return RHMC_OK;
}

int rhmc_ctx_set_image(rhmc_ctx* ctx, const double* D, int32_t rows, int32_t cols) {
  if (!ctx) return fail(RHMC_ERR_ARG, "ctx is NULL");
  if (!D) return fail(RHMC_ERR_ARG, "D is NULL");
  if (rows < 1 || cols < 1) return fail(RHMC_ERR_ARG, "rows/cols must be >= 1");
  if (rows != cols)
    return fail(RHMC_ERR_ARG, "rows must equal cols (reference gauss_PSF is square-only)");
  if ((int64_t)rows * cols > (1 << 26)) return fail(RHMC_ERR_ARG, "image too large");
  HIP_TRY(hipSetDevice(ctx->device));
  const size_t bytes = (size_t)rows * cols * sizeof(double);
  if (ctx->d_D && (ctx->rows * ctx->cols != rows * cols)) {
    HIP_TRY(hipFree(ctx->d_D));
    ctx->d_D = nullptr;
  }
  if (!ctx->d_D && hipMalloc(&ctx->d_D, bytes) != hipSuccess)
    return fail(RHMC_ERR_NOMEM, "hipMalloc image failed");
  HIP_TRY(hipMemcpyAsync(ctx->d_D, D, bytes, hipMemcpyHostToDevice, ctx->stream));
  ctx->rows = rows;
  ctx->cols = cols;
  int rc = refresh_image_f32(ctx);
  if (rc) return rc;
  HIP_TRY(hipStreamSynchronize(ctx->stream));
  return RHMC_OK;
}

int rhmc_ctx_create(int device, const double* D, int32_t rows, int32_t cols, rhmc_ctx** out) {
  if (!out) return fail(RHMC_ERR_ARG, "out is NULL");
  *out = nullptr;
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess || n == 0) return fail(RHMC_ERR_HIP, "no HIP device");
  if (device < 0 || device >= n) return fail(RHMC_ERR_ARG, "device out of range");
  HIP_TRY(hipSetDevice(device));
  rhmc_ctx* ctx = new rhmc_ctx();
  ctx->device = device;
  hipDeviceProp_t prop;
  if (hipGetDeviceProperties(&prop, device) != hipSuccess) {
    delete ctx;
    return fail(RHMC_ERR_HIP, "hipGetDeviceProperties failed");
  }
  ctx->max_lds = (int)prop.sharedMemPerBlock;
  ctx->n_cu = prop.multiProcessorCount;
  if (hipStreamCreateWithFlags(&ctx->stream, hipStreamNonBlocking) != hipSuccess) {
    delete ctx;
    return fail(RHMC_ERR_HIP, "hipStreamCreate failed");
  }
  int rc = D ? rhmc_ctx_set_image(ctx, D, rows, cols) : RHMC_OK;  // NULL: no image yet
  if (rc) {
    std::string keep = g_err;
    rhmc_ctx_destroy(ctx);
    g_err = keep;
    return rc;
  }
  *out = ctx;
  return RHMC_OK;
}

int rhmc_ctx_set_option(rhmc_ctx* ctx, int32_t option, int32_t value) {
  if (!ctx) return fail(RHMC_ERR_ARG, "ctx is NULL");
  switch (option) {
    case RHMC_OPT_KERNEL:
      if (value < RHMC_KERNEL_AUTO || value > RHMC_KERNEL_DENSE)
        return fail(RHMC_ERR_ARG, "unknown RHMC_KERNEL_* value " + std::to_string(value));
      ctx->kernel = value;
      return RHMC_OK;
    case RHMC_OPT_MH_FUSED:
      if (value != 0 && value != 1) return fail(RHMC_ERR_ARG, "RHMC_OPT_MH_FUSED must be 0 or 1");
      ctx->mh_fused = value;
      return RHMC_OK;
    case RHMC_OPT_PEAKS_FUSED:
      if (value != 0 && value != 1)
        return fail(RHMC_ERR_ARG, "RHMC_OPT_PEAKS_FUSED must be 0 or 1");
      ctx->peaks_fused = value;
      return RHMC_OK;
    case RHMC_OPT_DT_LANES:
      if (value != 0 && value != 64 && value != 256)
        return fail(RHMC_ERR_ARG, "RHMC_OPT_DT_LANES must be 0, 64 or 256");
      ctx->dt_lanes = value;
      return RHMC_OK;
    case RHMC_OPT_WINDOW_SPLIT:
      if (value != 0 && value != 1 && value != 2 && value != 4)
        return fail(RHMC_ERR_ARG, "RHMC_OPT_WINDOW_SPLIT must be 0, 1, 2 or 4");
      ctx->window_split = value;
      return RHMC_OK;
    case RHMC_OPT_TABLES:
      if (value != RHMC_TABLES_STREAM && value != RHMC_TABLES_STREAM_POISON)
        return fail(RHMC_ERR_ARG, "RHMC_OPT_TABLES must be 0 or 1");
      ctx->table_mode = value;
      return RHMC_OK;
    default:
      return fail(RHMC_ERR_ARG, "unknown option " + std::to_string(option));
  }
}

int rhmc_ctx_get_option(rhmc_ctx* ctx, int32_t option, int32_t* value) {
  if (!ctx || !value) return fail(RHMC_ERR_ARG, "NULL argument");
  switch (option) {
    case RHMC_OPT_KERNEL: *value = ctx->kernel; return RHMC_OK;
    case RHMC_OPT_MH_FUSED: *value = ctx->mh_fused; return RHMC_OK;
    case RHMC_OPT_WINDOW_SPLIT: *value = ctx->window_split; return RHMC_OK;
    case RHMC_OPT_TABLES: *value = ctx->table_mode; return RHMC_OK;
    case RHMC_OPT_PEAKS_FUSED: *value = ctx->peaks_fused; return RHMC_OK;
    case RHMC_OPT_DT_LANES: *value = ctx->dt_lanes; return RHMC_OK;
    default: return fail(RHMC_ERR_ARG, "unknown option " + std::to_string(option));
  }
}

int rhmc_ctx_image_device(rhmc_ctx* ctx, const double** d_image) {
  if (!ctx || !d_image) return fail(RHMC_ERR_ARG, "NULL argument");
  *d_image = ctx->d_D;
  return RHMC_OK;
}

void rhmc_ctx_destroy(rhmc_ctx* ctx) {
  if (!ctx) return;
  (void)hipSetDevice(ctx->device);
  if (ctx->stream) (void)hipStreamSynchronize(ctx->stream);
  if (ctx->d_D) (void)hipFree(ctx->d_D);
  if (ctx->d_Df) (void)hipFree(ctx->d_Df);
  if (ctx->d_flag) (void)hipFree(ctx->d_flag);
  if (ctx->scratch) (void)hipFree(ctx->scratch);
  if (ctx->mh_scratch) (void)hipFree(ctx->mh_scratch);
  if (ctx->h_pin) (void)hipHostFree(ctx->h_pin);
  if (ctx->dt_tab) (void)hipFree(ctx->dt_tab);
  if (!ctx->tabs.empty()) (void)hipDeviceSynchronize();  // tables may serve user streams
  for (auto& t : ctx->tabs)
    if (t.buf) t.buf->synced = true;  // user streams may be gone: no per-stream sync
  ctx->tabs.clear();
  if (ctx->stream) (void)hipStreamDestroy(ctx->stream);
  delete ctx;
}

int rhmc_ctx_synchronize(rhmc_ctx* ctx) {
  if (!ctx) return fail(RHMC_ERR_ARG, "ctx is NULL");
  HIP_TRY(hipSetDevice(ctx->device));
  HIP_TRY(hipStreamSynchronize(ctx->stream));
  return RHMC_OK;
}

int rhmc_leapfrog_device(rhmc_ctx* ctx, const rhmc_params* P, double* d_q, double* d_p,
                         int64_t n_chains, int32_t K, int32_t n_steps, int32_t* d_fp_iters,
                         int32_t* d_status, void* stream) {
  int rc = check_common(ctx, n_chains, K);
  if (rc) return rc;
  if (n_chains > 0 && (!d_q || !d_p)) return fail(RHMC_ERR_ARG, "q/p is NULL");
  hipStream_t s = stream ? (hipStream_t)stream : ctx->stream;
  return launch_leapfrog(ctx, P, d_q, d_p, n_chains, K, n_steps, d_fp_iters, d_status, s);
}

int rhmc_ragged_ok(rhmc_ctx* ctx, const rhmc_params* P, int32_t K, int32_t* ok) {
  if (!ctx) return fail(RHMC_ERR_ARG, "ctx is NULL");
  if (!ok) return fail(RHMC_ERR_ARG, "ok is NULL");
  if (!ctx->d_D) return fail(RHMC_ERR_ARG, "no image uploaded");
  Consts c;
  if (int rc = make_consts(P, &c)) return rc;
  *ok = ragged_family(select_in(ctx), c.use_Vc, c.inv_two_sig2, K) != 0 ? 1 : 0;
  return RHMC_OK;
}

int rhmc_leapfrog_ragged_device(rhmc_ctx* ctx, const rhmc_params* P, double* d_q, double* d_p,
                                int64_t ld, const int64_t* d_rows, const int32_t* d_K,
                                int64_t n, int32_t K_min, int32_t K_max, int32_t n_steps,
                                void* stream) {
  if (!ctx) return fail(RHMC_ERR_ARG, "ctx is NULL");
  if (!ctx->d_D) return fail(RHMC_ERR_ARG, "no image uploaded");
  if (n < 0 || n > ((int64_t)1 << 40)) return fail(RHMC_ERR_ARG, "bad n");
  if (n > 0 && (!d_q || !d_p || !d_K)) return fail(RHMC_ERR_ARG, "q, p or K is NULL");
  hipStream_t s = stream ? (hipStream_t)stream : ctx->stream;
  return launch_leapfrog_ragged(ctx, P, d_q, d_p, ld, d_rows, d_K, n, K_min, K_max, n_steps, s);
}

int rhmc_energy_ragged_device(rhmc_ctx* ctx, const rhmc_params* P, const double* d_q, int64_t ld,
                              const int64_t* d_rows, const int32_t* d_K, int64_t n,
                              int32_t K_min, int32_t K_max, int32_t f_pos, double* d_V,
                              void* stream) {
  if (!ctx) return fail(RHMC_ERR_ARG, "ctx is NULL");
  if (!ctx->d_D) return fail(RHMC_ERR_ARG, "no image uploaded");
  if (n < 0 || n > ((int64_t)1 << 40)) return fail(RHMC_ERR_ARG, "bad n");
  if (n > 0 && (!d_q || !d_K || !d_V)) return fail(RHMC_ERR_ARG, "q, K or V is NULL");
  hipStream_t s = stream ? (hipStream_t)stream : ctx->stream;
  return launch_energy_ragged(ctx, P, d_q, ld, d_rows, d_K, n, K_min, K_max, f_pos, d_V, s);
}

int rhmc_rows_copy_device(rhmc_ctx* ctx, const double* d_src, int64_t ld_src,
                          const int64_t* d_src_rows, double* d_dst, int64_t ld_dst,
                          const int64_t* d_dst_rows, int64_t n, int32_t width, void* stream) {
  if (!ctx) return fail(RHMC_ERR_ARG, "ctx is NULL");
  if (n < 0 || width < 0 || ld_src < width || ld_dst < width)
    return fail(RHMC_ERR_ARG, "rows copy: need n, width >= 0 and ld_src, ld_dst >= width");
  if (n == 0 || width == 0) return RHMC_OK;
  if (!d_src || !d_dst) return fail(RHMC_ERR_ARG, "rows copy: src or dst is NULL");
  HIP_TRY(hipSetDevice(ctx->device));
  hipStream_t s = stream ? (hipStream_t)stream : ctx->stream;
  RowsCopyArgs a{d_src, d_dst, d_src_rows, d_dst_rows, ld_src, ld_dst, n, width};
  const int64_t total = n * (int64_t)width;
  hipLaunchKernelGGL(rows_copy_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, a);
  HIP_TRY(hipGetLastError());
  return RHMC_OK;
}

int rhmc_kinetic_rows_device(rhmc_ctx* ctx, const rhmc_params* P, const double* d_q, double* d_p,
                             int64_t ld, const int32_t* d_K, const double* d_z,
                             const int64_t* d_zoff, int64_t n, double* d_T, void* stream) {
  if (!ctx) return fail(RHMC_ERR_ARG, "ctx is NULL");
  if (!P) return fail(RHMC_ERR_ARG, "params is NULL");
  if (n < 0 || ld < 3 || n > INT32_MAX) return fail(RHMC_ERR_ARG, "kinetic: bad n or ld");
  if (n == 0) return RHMC_OK;
  if (!d_q || !d_p || !d_K || !d_T || (d_z && !d_zoff))
    return fail(RHMC_ERR_ARG, "kinetic: q, p, K, T (or zoff with z) is NULL");
  HIP_TRY(hipSetDevice(ctx->device));
  hipStream_t s = stream ? (hipStream_t)stream : ctx->stream;
  KineticArgs a;
  a.q = d_q;
  a.p = d_p;
  a.z = d_z;
  a.zoff = d_zoff;
  a.K = d_K;
  a.T = d_T;
  a.ld = ld;
  a.n = n;
  a.g_ff2 = P->g_ff2;
  a.g_ff = P->g_ff;
  a.g_xx = P->g_xx;
  a.g0 = P->g0;
  a.g1 = P->g1;
  a.g2 = P->g2;
  a.B = P->B_count;
  a.f_low = P->f_low;
  if (ld <= 768)  // up to 256 stars: four chains per block
    hipLaunchKernelGGL((kinetic_rows_kernel<4, 768, 3>), dim3((unsigned)((n + 3) / 4)), dim3(256),
                       0, s, a);
  else  // up to 1024 stars: one chain per block (48 KB of LDS)
    hipLaunchKernelGGL((kinetic_rows_kernel<1, 3072, 5>), dim3((unsigned)n), dim3(64), 0, s, a);
  HIP_TRY(hipGetLastError());
  return RHMC_OK;
}

int rhmc_leapfrog(rhmc_ctx* ctx, const rhmc_params* P, double* q, double* p, int64_t n_chains,
                  int32_t K, int32_t n_steps, int32_t* fp_iters, int32_t* status) {
  int rc = check_common(ctx, n_chains, K);
  if (rc) return rc;
  if (n_chains == 0) return RHMC_OK;
  if (!q || !p) return fail(RHMC_ERR_ARG, "q/p is NULL");
  const size_t sb = (size_t)n_chains * 3 * K * sizeof(double);
  HIP_TRY(hipSetDevice(ctx->device));
  Staging st(ctx);
  const int iq = st.add(q, sb, Staging::kInOut), ip = st.add(p, sb, Staging::kInOut);
  const int ii = st.add(fp_iters, (size_t)n_chains * 2 * sizeof(int32_t), Staging::kOut);
  const int is = st.add(status, (size_t)n_chains * sizeof(int32_t), Staging::kOut);
  return st.run([&] {
    return launch_leapfrog(ctx, P, st.dev<double>(iq), st.dev<double>(ip), n_chains, K, n_steps,
                           st.dev<int32_t>(ii), st.dev<int32_t>(is), ctx->stream);
  });
}

int rhmc_gradient(rhmc_ctx* ctx, const rhmc_params* P, const double* q, double* grad,
                  int64_t n_chains, int32_t K, int32_t kind) {
  int rc = check_common(ctx, n_chains, K);
  if (rc) return rc;
  if (kind != 0 && kind != 1) return fail(RHMC_ERR_ARG, "kind must be 0 (dVdq) or 1 (dphidq)");
  if (n_chains == 0) return RHMC_OK;
  if (!q || !grad) return fail(RHMC_ERR_ARG, "q/grad is NULL");
  Consts c;
  if ((rc = make_consts(P, &c))) return rc;
  Plan pl;
  if ((rc = plan_for(ctx, c, Op::Gradient, K, n_chains, &pl))) return rc;
  const size_t sb = (size_t)n_chains * 3 * K * sizeof(double);
  HIP_TRY(hipSetDevice(ctx->device));
  Staging st(ctx);
  const int iq = st.add(q, sb, Staging::kIn), ig = st.add(grad, sb, Staging::kOut);
  return st.run([&] {
    return launch_gradient(ctx, pl, c, st.dev<double>(iq), st.dev<double>(ig), n_chains, K, kind,
                           ctx->stream);
  });
}

int rhmc_energy_device(rhmc_ctx* ctx, const rhmc_params* P, const double* d_q, const double* d_p,
                       double* d_V, double* d_T, int64_t n_chains, int32_t K, int32_t f_pos,
                       void* stream) {
  int rc = check_common(ctx, n_chains, K);
  if (rc) return rc;
  if (n_chains == 0) return RHMC_OK;
  if (!d_q) return fail(RHMC_ERR_ARG, "q is NULL");
  if (d_T && !d_p) return fail(RHMC_ERR_ARG, "T requested but p is NULL");
  Consts c;
  if ((rc = make_consts(P, &c))) return rc;
  HIP_TRY(hipSetDevice(ctx->device));
  hipStream_t s = stream ? (hipStream_t)stream : ctx->stream;
  return launch_energy(ctx, c, d_q, d_T ? d_p : nullptr, d_V, d_T, n_chains, K, f_pos, s);
}

int rhmc_energy(rhmc_ctx* ctx, const rhmc_params* P, const double* q, const double* p, double* V,
                double* T, int64_t n_chains, int32_t K, int32_t f_pos) {
  int rc = check_common(ctx, n_chains, K);
  if (rc) return rc;
  if (n_chains == 0) return RHMC_OK;
  if (!q) return fail(RHMC_ERR_ARG, "q is NULL");
  if (T && !p) return fail(RHMC_ERR_ARG, "T requested but p is NULL");
  Consts c;
  if ((rc = make_consts(P, &c))) return rc;
  const size_t sb = (size_t)n_chains * 3 * K * sizeof(double);
  const size_t eb = (size_t)n_chains * sizeof(double);
  HIP_TRY(hipSetDevice(ctx->device));
  Staging st(ctx);  // p only for T; an output not asked for has no part (NULL to the kernel)
  const int iq = st.add(q, sb, Staging::kIn), ip = st.add(p, T ? sb : 0, Staging::kIn);
  const int iV = st.add(V, V ? eb : 0, Staging::kOut), iT = st.add(T, T ? eb : 0, Staging::kOut);
  return st.run([&] {
    return launch_energy(ctx, c, st.dev<double>(iq), st.dev<double>(ip), st.dev<double>(iV),
                         st.dev<double>(iT), n_chains, K, f_pos, ctx->stream);
  });
}

int rhmc_mh_scheduled_device(rhmc_ctx* ctx, const rhmc_params* P, double* d_q,
                             int64_t n_chains, int32_t K, int32_t n_iter, int32_t n_steps,
                             int32_t f_pos, const double* d_z, const double* d_u, uint64_t seed,
                             const rhmc_mh_record* rec, const rhmc_mh_schedule* sched,
                             void* stream) {
  int rc = check_common(ctx, n_chains, K);
  if (rc) return rc;
  if (n_chains > 0 && !d_q) return fail(RHMC_ERR_ARG, "q is NULL");
  HIP_TRY(hipSetDevice(ctx->device));
  hipStream_t s = stream ? (hipStream_t)stream : ctx->stream;
  return run_mh(ctx, P, d_q, n_chains, K, n_iter, n_steps, f_pos, d_z, d_u, seed, rec, s, sched);
}

int rhmc_mh_device(rhmc_ctx* ctx, const rhmc_params* P, double* d_q, int64_t n_chains,
                   int32_t K, int32_t n_iter, int32_t n_steps, int32_t f_pos, const double* d_z,
                   const double* d_u, uint64_t seed, const rhmc_mh_record* rec, void* stream) {
  return rhmc_mh_scheduled_device(ctx, P, d_q, n_chains, K, n_iter, n_steps, f_pos, d_z, d_u,
                                  seed, rec, nullptr, stream);
}

int rhmc_mh(rhmc_ctx* ctx, const rhmc_params* P, double* q, int64_t n_chains, int32_t K,
            int32_t n_iter, int32_t n_steps, int32_t f_pos, const double* z, const double* u,
            uint64_t seed, const rhmc_mh_record* rec) {
  return rhmc_mh_scheduled(ctx, P, q, n_chains, K, n_iter, n_steps, f_pos, z, u, seed, rec,
                           nullptr);
}

int rhmc_mh_scheduled(rhmc_ctx* ctx, const rhmc_params* P, double* q, int64_t n_chains,
                      int32_t K, int32_t n_iter, int32_t n_steps, int32_t f_pos, const double* z,
                      const double* u, uint64_t seed, const rhmc_mh_record* rec,
                      const rhmc_mh_schedule* sched) {
  int rc = check_common(ctx, n_chains, K);
  if (rc) return rc;
  if (n_chains == 0 || n_iter == 0) return RHMC_OK;
  if (!q) return fail(RHMC_ERR_ARG, "q is NULL");
  if (n_iter < 0) return fail(RHMC_ERR_ARG, "n_iter < 0");
  const size_t sb = (size_t)n_chains * 3 * K * sizeof(double);
  const size_t eb = (size_t)n_iter * n_chains * sizeof(double);
  const size_t ab = (size_t)n_iter * n_chains * sizeof(int32_t);
  const rhmc_mh_record none{nullptr, nullptr, nullptr, nullptr, nullptr};
  const rhmc_mh_record& r = rec ? *rec : none;
  HIP_TRY(hipSetDevice(ctx->device));
  Staging st(ctx);  // a record not asked for, or no host randoms: no part, NULL to the kernels
  const int iq = st.add(q, sb, Staging::kInOut);
  const int iz = st.add(z, z ? (size_t)n_iter * sb : 0, Staging::kIn);
  const int iu = st.add(u, u ? eb : 0, Staging::kIn);
  const int iqc = st.add(r.q_chain, r.q_chain ? (size_t)n_iter * sb : 0, Staging::kOut);
  const int iE = st.add(r.E_chain, r.E_chain ? eb : 0, Staging::kOut);
  const int iV = st.add(r.V_chain, r.V_chain ? eb : 0, Staging::kOut);
  const int iT = st.add(r.T_chain, r.T_chain ? eb : 0, Staging::kOut);
  const int ia = st.add(r.accept, r.accept ? ab : 0, Staging::kOut);
  return st.run([&] {
    const rhmc_mh_record drec{st.dev<double>(iqc), st.dev<double>(iE), st.dev<double>(iV),
                              st.dev<double>(iT), st.dev<int32_t>(ia)};
    return run_mh(ctx, P, st.dev<double>(iq), n_chains, K, n_iter, n_steps, f_pos,
                  st.dev<double>(iz), st.dev<double>(iu), seed, &drec, ctx->stream, sched);
  });
}

int rhmc_integrate_device(rhmc_ctx* ctx, const rhmc_params* P, int32_t solver, double* d_q,
                          double* d_p, int64_t n_chains, int32_t K, int32_t n_steps,
                          int32_t f_pos, int32_t* d_status, void* stream) {
  int rc = check_common(ctx, n_chains, K);
  if (rc) return rc;
  if (n_chains > 0 && (!d_q || !d_p)) return fail(RHMC_ERR_ARG, "q/p is NULL");
  hipStream_t s = stream ? (hipStream_t)stream : ctx->stream;
  return launch_integrate(ctx, P, solver, d_q, d_p, n_chains, K, n_steps, f_pos, d_status, s);
}

int rhmc_integrate(rhmc_ctx* ctx, const rhmc_params* P, int32_t solver, double* q, double* p,
                   int64_t n_chains, int32_t K, int32_t n_steps, int32_t f_pos,
                   int32_t* status) {
  int rc = check_common(ctx, n_chains, K);
  if (rc) return rc;
  if (n_chains == 0) return RHMC_OK;
  if (!q || !p) return fail(RHMC_ERR_ARG, "q/p is NULL");
  const size_t sb = (size_t)n_chains * 3 * K * sizeof(double);
  HIP_TRY(hipSetDevice(ctx->device));
  Staging st(ctx);
  const int iq = st.add(q, sb, Staging::kInOut), ip = st.add(p, sb, Staging::kInOut);
  const int is = st.add(status, (size_t)n_chains * sizeof(int32_t), Staging::kOut);
  return st.run([&] {
    return launch_integrate(ctx, P, solver, st.dev<double>(iq), st.dev<double>(ip), n_chains, K,
                            n_steps, f_pos, st.dev<int32_t>(is), ctx->stream);
  });
}

int rhmc_hmc_random_device(rhmc_ctx* ctx, const rhmc_params* P, const double* d_dt,
                           double* d_q, double* d_p, const int32_t* d_steps, int64_t n_chains,
                           int32_t K, int32_t* d_status, void* stream) {
  int rc = check_common(ctx, n_chains, K);
  if (rc) return rc;
  if (n_chains > 0 && (!d_q || !d_p)) return fail(RHMC_ERR_ARG, "q/p is NULL");
  hipStream_t s = stream ? (hipStream_t)stream : ctx->stream;
  return launch_hmc_random(ctx, P, d_dt, d_q, d_p, d_steps, n_chains, K, d_status, s);
}

int rhmc_hmc_random(rhmc_ctx* ctx, const rhmc_params* P, const double* dt, double* q, double* p,
                    const int32_t* steps, int64_t n_chains, int32_t K, int32_t* status) {
  int rc = check_common(ctx, n_chains, K);
  if (rc) return rc;
  if (n_chains == 0) return RHMC_OK;
  if (!q || !p || !dt || !steps) return fail(RHMC_ERR_ARG, "q/p/dt/steps is NULL");
  for (int64_t i = 0; i < n_chains; ++i)
    if (steps[i] < 1) return fail(RHMC_ERR_ARG, "steps[i] must be >= 1");
  const size_t sb = (size_t)n_chains * 3 * K * sizeof(double);
  const size_t tb = (size_t)n_chains * sizeof(int32_t);
  HIP_TRY(hipSetDevice(ctx->device));
  Staging st(ctx);
  const int iq = st.add(q, sb, Staging::kInOut), ip = st.add(p, sb, Staging::kInOut);
  const int is = st.add(status, tb, Staging::kOut), in = st.add(steps, tb, Staging::kIn);
  const int id = st.add(dt, (size_t)3 * K * sizeof(double), Staging::kIn);
  return st.run([&] {
    return launch_hmc_random(ctx, P, st.dev<double>(id), st.dev<double>(iq), st.dev<double>(ip),
                             st.dev<int32_t>(in), n_chains, K, st.dev<int32_t>(is), ctx->stream);
  });
}

int rhmc_diag_random_device(rhmc_ctx* ctx, const rhmc_params* P, const rhmc_diag_opts* opts,
                            double* d_q, double* d_p, const int32_t* d_steps, int64_t n_chains,
                            int32_t K, int32_t* d_status, double* d_trace, void* stream) {
  if (int rc = check_diag(ctx, P, opts, d_q, d_p, d_steps, n_chains, K, d_trace, false)) return rc;
  if (n_chains == 0) return RHMC_OK;
  hipStream_t s = stream ? (hipStream_t)stream : ctx->stream;
  return launch_diag_random(ctx, P, opts, d_q, d_p, d_steps, n_chains, K, d_status, d_trace, s);
}

int rhmc_diag_random(rhmc_ctx* ctx, const rhmc_params* P, const rhmc_diag_opts* opts, double* q,
                     double* p, const int32_t* steps, int64_t n_chains, int32_t K,
                     int32_t* status, double* trace) {
  if (int rc = check_diag(ctx, P, opts, q, p, steps, n_chains, K, trace, true)) return rc;
  if (n_chains == 0) return RHMC_OK;
  const size_t sb = (size_t)n_chains * 3 * K * sizeof(double);
  const size_t tb = (size_t)n_chains * sizeof(int32_t);
  HIP_TRY(hipSetDevice(ctx->device));
  Staging st(ctx);  // rows past a chain's trajectory come back as they went in
  const int iq = st.add(q, sb, Staging::kInOut), ip = st.add(p, sb, Staging::kInOut);
  const int is = st.add(status, status ? tb : 0, Staging::kOut);
  const int in = st.add(steps, tb, Staging::kIn);
  const int it = st.add(trace, trace ? sb * (size_t)opts->trace_rows : 0, Staging::kInOut);
  return st.run([&] {
    return launch_diag_random(ctx, P, opts, st.dev<double>(iq), st.dev<double>(ip),
                              st.dev<int32_t>(in), n_chains, K, st.dev<int32_t>(is),
                              st.dev<double>(it), ctx->stream);
  });
}

int rhmc_hess_derivs_device(rhmc_ctx* ctx, const rhmc_params* P, const double* d_q,
                            double* d_dVdq, double* d_dVdqq, double* d_dVdqqq, double* d_V,
                            int64_t n_chains, int32_t K, void* stream) {
  if (int rc = check_hess(ctx, P, nullptr, d_q, nullptr, nullptr, n_chains, K, false, false))
    return rc;
  if (n_chains == 0) return RHMC_OK;
  hipStream_t s = stream ? (hipStream_t)stream : ctx->stream;
  return launch_hess(ctx, P, nullptr, const_cast<double*>(d_q), nullptr, nullptr, n_chains, K,
                     nullptr, nullptr, d_dVdq, d_dVdqq, d_dVdqqq, d_V, s);
}

int rhmc_hess_derivs(rhmc_ctx* ctx, const rhmc_params* P, const double* q, double* dVdq,
                     double* dVdqq, double* dVdqqq, double* V, int64_t n_chains, int32_t K) {
  if (int rc = check_hess(ctx, P, nullptr, q, nullptr, nullptr, n_chains, K, false, true))
    return rc;
  if (n_chains == 0) return RHMC_OK;
  const size_t sb = (size_t)n_chains * 3 * K * sizeof(double);
  HIP_TRY(hipSetDevice(ctx->device));
  Staging st(ctx);  // an output not asked for has no part (NULL to the kernel)
  const int iq = st.add(q, sb, Staging::kIn);
  const int i1 = st.add(dVdq, dVdq ? sb : 0, Staging::kOut);
  const int i2 = st.add(dVdqq, dVdqq ? sb : 0, Staging::kOut);
  const int i3 = st.add(dVdqqq, dVdqqq ? sb : 0, Staging::kOut);
  const int iV = st.add(V, V ? (size_t)n_chains * sizeof(double) : 0, Staging::kOut);
  return st.run([&] {
    return launch_hess(ctx, P, nullptr, st.dev<double>(iq), nullptr, nullptr, n_chains, K,
                       nullptr, nullptr, st.dev<double>(i1), st.dev<double>(i2),
                       st.dev<double>(i3), st.dev<double>(iV), ctx->stream);
  });
}

int rhmc_hess_random_device(rhmc_ctx* ctx, const rhmc_params* P, const rhmc_hess_opts* opts,
                            double* d_q, double* d_p, const int32_t* d_steps, int64_t n_chains,
                            int32_t K, int32_t* d_status, int32_t* d_steps_done, double* d_dVdq,
                            double* d_dVdqq, double* d_dVdqqq, void* stream) {
  if (int rc = check_hess(ctx, P, opts, d_q, d_p, d_steps, n_chains, K, true, false)) return rc;
  if (n_chains == 0) return RHMC_OK;
  hipStream_t s = stream ? (hipStream_t)stream : ctx->stream;
  return launch_hess(ctx, P, opts, d_q, d_p, d_steps, n_chains, K, d_status, d_steps_done,
                     d_dVdq, d_dVdqq, d_dVdqqq, nullptr, s);
}

int rhmc_hess_random(rhmc_ctx* ctx, const rhmc_params* P, const rhmc_hess_opts* opts, double* q,
                     double* p, const int32_t* steps, int64_t n_chains, int32_t K,
                     int32_t* status, int32_t* steps_done, double* dVdq, double* dVdqq,
                     double* dVdqqq) {
  if (int rc = check_hess(ctx, P, opts, q, p, steps, n_chains, K, true, true)) return rc;
  if (n_chains == 0) return RHMC_OK;
  const size_t sb = (size_t)n_chains * 3 * K * sizeof(double);
  const size_t tb = (size_t)n_chains * sizeof(int32_t);
  HIP_TRY(hipSetDevice(ctx->device));
  Staging st(ctx);  // an output not asked for has no part (NULL to the kernel)
  const int iq = st.add(q, sb, Staging::kInOut), ip = st.add(p, sb, Staging::kInOut);
  const int in = st.add(steps, tb, Staging::kIn);
  const int is = st.add(status, status ? tb : 0, Staging::kOut);
  const int id = st.add(steps_done, steps_done ? tb : 0, Staging::kOut);
  const int i1 = st.add(dVdq, dVdq ? sb : 0, Staging::kOut);
  const int i2 = st.add(dVdqq, dVdqq ? sb : 0, Staging::kOut);
  const int i3 = st.add(dVdqqq, dVdqqq ? sb : 0, Staging::kOut);
  return st.run([&] {
    return launch_hess(ctx, P, opts, st.dev<double>(iq), st.dev<double>(ip), st.dev<int32_t>(in),
                       n_chains, K, st.dev<int32_t>(is), st.dev<int32_t>(id), st.dev<double>(i1),
                       st.dev<double>(i2), st.dev<double>(i3), nullptr, ctx->stream);
  });
}

int rhmc_find_peaks_device(rhmc_ctx* ctx, const rhmc_params* P, const rhmc_peaks_opts* opts,
                           double* d_q, int64_t n, int32_t* d_steps, int32_t* d_status,
                           double* d_V, void* stream) {
  if (int rc = check_peaks(ctx, P, opts, d_q, n)) return rc;
  if (n == 0) return RHMC_OK;
  hipStream_t s = stream ? (hipStream_t)stream : ctx->stream;
  return launch_find_peaks(ctx, P, opts, d_q, n, d_steps, d_status, d_V, s);
}

int rhmc_find_peaks(rhmc_ctx* ctx, const rhmc_params* P, const rhmc_peaks_opts* opts, double* q,
                    int64_t n, int32_t* steps, int32_t* status, double* V) {
  if (int rc = check_peaks(ctx, P, opts, q, n)) return rc;
  if (n == 0) return RHMC_OK;
  HIP_TRY(hipSetDevice(ctx->device));
  Staging st(ctx);  // an output not asked for has no part (NULL to the kernels)
  const int iq = st.add(q, (size_t)n * 3 * sizeof(double), Staging::kInOut);
  const int is = st.add(steps, steps ? (size_t)n * sizeof(int32_t) : 0, Staging::kOut);
  const int it = st.add(status, status ? (size_t)n * sizeof(int32_t) : 0, Staging::kOut);
  const int iV = st.add(V, V ? (size_t)n * sizeof(double) : 0, Staging::kOut);
  return st.run([&] {
    return launch_find_peaks(ctx, P, opts, st.dev<double>(iq), n, st.dev<int32_t>(is),
                             st.dev<int32_t>(it), st.dev<double>(iV), ctx->stream);
  });
}

int rhmc_dt_trials_device(rhmc_ctx* ctx, const rhmc_params* P, const rhmc_dt_opts* opts,
                          const double* d_bg, int32_t n_bg, const int32_t* d_bg_index,
                          const double* d_q0, const double* d_dt, const int32_t* d_flux_only,
                          int64_t n, const double* d_z, const int32_t* d_steps,
                          const double* d_lnu, uint64_t seed, const uint64_t* d_stream_id,
                          int32_t* d_n_accept, const rhmc_dt_record* rec, void* stream) {
  if (int rc = check_dt(ctx, P, opts, d_bg, n_bg, d_bg_index, d_q0, d_dt, n, d_z, d_steps, d_lnu,
                        d_stream_id, false))
    return rc;
  if (n == 0) return RHMC_OK;
  hipStream_t s = stream ? (hipStream_t)stream : ctx->stream;
  const DtCall k{d_bg, n_bg, d_bg_index, d_q0, d_dt, d_flux_only, n, d_z, d_steps, d_lnu, seed,
                 d_stream_id, d_n_accept, rec ? *rec : rhmc_dt_record{}};
  return launch_dt_trials(ctx, P, opts, k, s);
}

int rhmc_dt_trials(rhmc_ctx* ctx, const rhmc_params* P, const rhmc_dt_opts* opts,
                   const double* bg, int32_t n_bg, const int32_t* bg_index, const double* q0,
                   const double* dt, const int32_t* flux_only, int64_t n, const double* z,
                   const int32_t* steps, const double* lnu, uint64_t seed,
                   const uint64_t* stream_id, int32_t* n_accept, const rhmc_dt_record* rec) {
  if (int rc = check_dt(ctx, P, opts, bg, n_bg, bg_index, q0, dt, n, z, steps, lnu, stream_id,
                        true))
    return rc;
  if (n == 0) return RHMC_OK;
  HIP_TRY(hipSetDevice(ctx->device));
  const size_t npix = (size_t)ctx->rows * ctx->cols, ni = (size_t)n * opts->n_iter;
  const rhmc_dt_record r = rec ? *rec : rhmc_dt_record{};
  Staging st(ctx);  // an array not given has no part (NULL to the kernel)
  const int ibg = st.add(bg, (size_t)n_bg * npix * sizeof(double), Staging::kIn);
  const int ibi = st.add(bg_index, (size_t)n * sizeof(int32_t), Staging::kIn);
  const int iq0 = st.add(q0, (size_t)n * 3 * sizeof(double), Staging::kIn);
  const int idt = st.add(dt, (size_t)n * 3 * sizeof(double), Staging::kIn);
  const int ifo = st.add(flux_only, flux_only ? (size_t)n * sizeof(int32_t) : 0, Staging::kIn);
  const int iz = st.add(z, z ? ni * 3 * sizeof(double) : 0, Staging::kIn);
  const int ist = st.add(steps, steps ? ni * sizeof(int32_t) : 0, Staging::kIn);
  const int ilu = st.add(lnu, lnu ? ni * sizeof(double) : 0, Staging::kIn);
  const int isi = st.add(stream_id, stream_id ? (size_t)n * sizeof(uint64_t) : 0, Staging::kIn);
  const int ina = st.add(n_accept, n_accept ? (size_t)n * sizeof(int32_t) : 0, Staging::kOut);
  const int rdE = st.add(r.dE, r.dE ? ni * sizeof(double) : 0, Staging::kOut);
  const int rac = st.add(r.accept, r.accept ? ni * sizeof(int32_t) : 0, Staging::kOut);
  const int rq = st.add(r.q, r.q ? ni * 3 * sizeof(double) : 0, Staging::kOut);
  const int rz = st.add(r.z, r.z ? ni * 3 * sizeof(double) : 0, Staging::kOut);
  const int rst = st.add(r.steps, r.steps ? ni * sizeof(int32_t) : 0, Staging::kOut);
  const int rlu = st.add(r.lnu, r.lnu ? ni * sizeof(double) : 0, Staging::kOut);
  return st.run([&] {
    const DtCall k{st.dev<double>(ibg), n_bg, st.dev<int32_t>(ibi), st.dev<double>(iq0),
                   st.dev<double>(idt), st.dev<int32_t>(ifo), n, st.dev<double>(iz),
                   st.dev<int32_t>(ist), st.dev<double>(ilu), seed, st.dev<uint64_t>(isi),
                   st.dev<int32_t>(ina),
                   rhmc_dt_record{st.dev<double>(rdE), st.dev<int32_t>(rac), st.dev<double>(rq),
                                  st.dev<double>(rz), st.dev<int32_t>(rst), st.dev<double>(rlu)}};
    return launch_dt_trials(ctx, P, opts, k, ctx->stream);
  });
}

int rhmc_chain_device(rhmc_ctx* ctx, const rhmc_params* P, const rhmc_chain_opts* opts,
                      const double* d_dt, double* d_q, int64_t n, int32_t K, const double* d_z,
                      const int32_t* d_steps, const double* d_lnu, uint64_t seed,
                      const uint64_t* d_stream_id, const rhmc_chain_record* rec, void* stream) {
  if (int rc = check_chain(ctx, P, opts, d_dt, d_q, n, K, d_z, d_steps, d_lnu, false)) return rc;
  if (n == 0) return RHMC_OK;
  hipStream_t s = stream ? (hipStream_t)stream : ctx->stream;
  const ChainCall k{d_dt, d_q, n, K, d_z, d_steps, d_lnu, seed, d_stream_id,
                    rec ? *rec : rhmc_chain_record{}};
  return opts->metric == RHMC_CHAIN_DIAG ? run_chain<true>(ctx, P, opts, k, s)
                                         : run_chain<false>(ctx, P, opts, k, s);
}

int rhmc_chain(rhmc_ctx* ctx, const rhmc_params* P, const rhmc_chain_opts* opts, const double* dt,
               double* q, int64_t n, int32_t K, const double* z, const int32_t* steps,
               const double* lnu, uint64_t seed, const uint64_t* stream_id,
               const rhmc_chain_record* rec) {
  if (int rc = check_chain(ctx, P, opts, dt, q, n, K, z, steps, lnu, true)) return rc;
  if (n == 0) return RHMC_OK;
  HIP_TRY(hipSetDevice(ctx->device));
  const bool diag = opts->metric == RHMC_CHAIN_DIAG;
  const size_t sb = (size_t)n * 3 * K * sizeof(double);
  const size_t ni = (size_t)n * opts->n_iter, ni1 = ni + (size_t)n;
  const rhmc_chain_record r = rec ? *rec : rhmc_chain_record{};
  Staging st(ctx);  // an array not given has no part (NULL to the kernels)
  const int iq = st.add(q, sb, Staging::kInOut);
  const int idt = st.add(dt, (dt && !diag) ? (size_t)3 * K * sizeof(double) : 0, Staging::kIn);
  const int iz = st.add(z, z ? (size_t)(opts->n_iter + 1) * sb : 0, Staging::kIn);
  const int ist = st.add(steps, steps ? ni * sizeof(int32_t) : 0, Staging::kIn);
  const int ilu = st.add(lnu, lnu ? ni * sizeof(double) : 0, Staging::kIn);
  const int isi = st.add(stream_id, stream_id ? (size_t)n * sizeof(uint64_t) : 0, Staging::kIn);
  const int rq = st.add(r.q_chain, r.q_chain ? (size_t)(opts->n_iter + 1) * sb : 0, Staging::kOut);
  const int rE = st.add(r.E_chain, r.E_chain ? ni1 * sizeof(double) : 0, Staging::kOut);
  const int rdE = st.add(r.dE_chain, r.dE_chain ? ni1 * sizeof(double) : 0, Staging::kOut);
  const int rac = st.add(r.accept, r.accept ? ni * sizeof(int32_t) : 0, Staging::kOut);
  const int rst = st.add(r.status, r.status ? ni * sizeof(int32_t) : 0, Staging::kOut);
  const int rz = st.add(r.z, r.z ? (size_t)(opts->n_iter + 1) * sb : 0, Staging::kOut);
  const int rsp = st.add(r.steps, r.steps ? ni * sizeof(int32_t) : 0, Staging::kOut);
  const int rlu = st.add(r.lnu, r.lnu ? ni * sizeof(double) : 0, Staging::kOut);
  return st.run([&] {
    const ChainCall k{st.dev<double>(idt), st.dev<double>(iq), n, K, st.dev<double>(iz),
                      st.dev<int32_t>(ist), st.dev<double>(ilu), seed, st.dev<uint64_t>(isi),
                      rhmc_chain_record{st.dev<double>(rq), st.dev<double>(rE),
                                        st.dev<double>(rdE), st.dev<int32_t>(rac),
                                        st.dev<int32_t>(rst), st.dev<double>(rz),
                                        st.dev<int32_t>(rsp), st.dev<double>(rlu)}};
    return diag ? run_chain<true>(ctx, P, opts, k, ctx->stream)
                : run_chain<false>(ctx, P, opts, k, ctx->stream);
  });
}

int rhmc_gen_image_device(rhmc_ctx* ctx, const rhmc_params* P, const double* d_q, int32_t K,
                          int32_t rows, int32_t cols, int32_t n_real, uint64_t seed,
                          double* d_out, void* stream) {
  if (!ctx) return fail(RHMC_ERR_ARG, "ctx is NULL");
  hipStream_t s = stream ? (hipStream_t)stream : ctx->stream;
  return launch_gen_image(ctx, P, d_q, K, rows, cols, n_real, seed, d_out, s);
}

int rhmc_gen_image(rhmc_ctx* ctx, const rhmc_params* P, const double* q, int32_t K, int32_t rows,
                   int32_t cols, int32_t n_real, uint64_t seed, double* out, int32_t install) {
  if (!ctx) return fail(RHMC_ERR_ARG, "ctx is NULL");
  if (!out && !install) return fail(RHMC_ERR_ARG, "out is NULL and install == 0");
  if (K < 0 || K > (1 << 20)) return fail(RHMC_ERR_ARG, "K must be in [0, 2^20]");
  if (K > 0 && !q) return fail(RHMC_ERR_ARG, "q is NULL");
  if (rows < 1 || cols < 1) return fail(RHMC_ERR_ARG, "rows/cols must be >= 1");
  if (n_real < 0) return fail(RHMC_ERR_ARG, "n_real < 0");
  if (install && rows != cols)
    return fail(RHMC_ERR_ARG, "rows must equal cols to install the image");
  if (install && (int64_t)rows * cols > (1 << 26)) return fail(RHMC_ERR_ARG, "image too large");
  const int64_t npix = (int64_t)rows * cols;
  const int64_t nimg = n_real > 0 ? n_real : 1;
  if (npix * nimg > ((int64_t)1 << 36)) return fail(RHMC_ERR_ARG, "rows*cols*n_real too large");
  HIP_TRY(hipSetDevice(ctx->device));
  Staging st(ctx);
  const int iq = st.add(q, (size_t)3 * K * sizeof(double), Staging::kIn);
  const int io = st.add(out, (size_t)(npix * nimg) * sizeof(double), Staging::kOut);
  return st.run([&] {
    double* dout = st.dev<double>(io);
    int rc = launch_gen_image(ctx, P, st.dev<double>(iq), K, rows, cols, n_real, seed, dout,
                              ctx->stream);
    if (rc || !install) return rc;
    // image 0 becomes the context's data image (stays on the device)
    const size_t bytes = (size_t)npix * sizeof(double);
    if (ctx->d_D && (int64_t)ctx->rows * ctx->cols != npix) {
      HIP_TRY(hipStreamSynchronize(ctx->stream));
      HIP_TRY(hipFree(ctx->d_D));
      ctx->d_D = nullptr;
    }
    if (!ctx->d_D && hipMalloc(&ctx->d_D, bytes) != hipSuccess)
      return fail(RHMC_ERR_NOMEM, "hipMalloc image failed");
    HIP_TRY(hipMemcpyAsync(ctx->d_D, dout, bytes, hipMemcpyDeviceToDevice, ctx->stream));
    ctx->rows = rows;
    ctx->cols = cols;
    return refresh_image_f32(ctx);
  });
}
}  // extern "C"
