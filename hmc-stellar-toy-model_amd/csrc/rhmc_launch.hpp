// rhmc_launch.hpp — the host side between the C-ABI (rhmc_kernels.hip) and
// the kernels: one builder per kernel-argument struct, one launcher per
// kernel family, and the launch_* function of every operation, which asks
// rhmc_select.hpp for a Plan and picks the family's launcher.  A launcher adds
// the launch shape (workgroup, LDS bytes, grid, table lease) and calls one
// switch of rhmc_dispatch.hpp, which turns the plan into template arguments;
// its functor enqueues the kernel.  No template argument is decided here.
// Included by rhmc_kernels.hip alone, after rhmc_ctx, fail() and HIP_TRY:
// template kernels are launched from the translation unit that instantiates them.
#pragma once
#include "rhmc_dispatch.hpp"

namespace {

SelectIn select_in(const rhmc_ctx* ctx) {
  return SelectIn{ctx->rows,  ctx->cols,   ctx->img_f32,  ctx->max_lds,     ctx->n_cu,
                  ctx->kernel, ctx->mh_fused, ctx->window_split, ctx->peaks_fused,
                  ctx->dt_lanes};
}

// The plan of one call; an unsupported configuration is the error here.
int plan_for(const rhmc_ctx* ctx, const Consts& c, Op op, int K, int64_t n, Plan* pl) {
  *pl = select(select_in(ctx), c.use_Vc, c.inv_two_sig2, op, K, n);
  return pl->family == Family::Unsupported ? fail(RHMC_ERR_UNSUPPORTED, pl->message) : RHMC_OK;
}

int launch_status() {
  HIP_TRY(hipGetLastError());
  return RHMC_OK;
}

// ---------------------------------------------------------------------------
// Device buffers the context keeps
// ---------------------------------------------------------------------------

// Grow a device buffer to `need` bytes (contents are not kept).  A failed
// allocation returns RHMC_ERR_NOMEM without a message: the caller names the buffer.
int grow(void** ptr, size_t* bytes, size_t need) {
  if (need <= *bytes) return RHMC_OK;
  if (*ptr) HIP_TRY(hipFree(*ptr));
  *ptr = nullptr;
  *bytes = 0;
  if (hipMalloc(ptr, need) != hipSuccess) return RHMC_ERR_NOMEM;
  *bytes = need;
  return RHMC_OK;
}

int ensure_scratch(rhmc_ctx* ctx, size_t bytes) {
  const int rc = grow(&ctx->scratch, &ctx->scratch_bytes, bytes);
  if (rc == RHMC_ERR_NOMEM)
    return fail(RHMC_ERR_NOMEM, "hipMalloc scratch " + std::to_string(bytes) + " B failed");
  return rc;
}

int ensure_mh_scratch(rhmc_ctx* ctx, size_t bytes) {
  const int rc = grow(&ctx->mh_scratch, &ctx->mh_scratch_bytes, bytes);
  return rc == RHMC_ERR_NOMEM ? fail(RHMC_ERR_NOMEM, "hipMalloc MH scratch failed") : rc;
}

// WinGG's per-chain factor tables (from kWinGlobalFromK stars): one buffer per
// (context, stream), grown on demand and kept until rhmc_ctx_destroy.  Launches
// on one stream run in order, so they can share it.  The caller keeps `lease`
// alive until its launch is enqueued: a grow by another thread on the same
// stream then replaces the context's buffer, and the old one is released only
// when its last lease goes (after a sync of its stream).  Every region a launch
// uses is written by that launch before it is read (win_build_tables,
// win_build_ey), which RHMC_TABLES_STREAM_POISON checks by filling the buffer
// with 0xFF bytes ahead of the launch.
using TableLease = std::shared_ptr<rhmc_ctx::TabBuf>;

int work_tables(const rhmc_ctx* ctx, const Plan& pl, int K, int64_t n, hipStream_t st,
                double** out, TableLease* lease) {
  *out = nullptr;
  lease->reset();
  if (pl.policy != Policy::WinGG || n <= 0) return RHMC_OK;
  const size_t bytes = (size_t)n * WinGG::work_doubles(K) * sizeof(double);
  const bool poison = ctx->table_mode == RHMC_TABLES_STREAM_POISON;
  std::lock_guard<std::mutex> lk(ctx->tab_mu);
  rhmc_ctx::StreamTables* t = nullptr;
  for (auto& e : ctx->tabs)
    if (e.s == st) t = &e;
  if (!t || !t->buf || t->buf->bytes < bytes) {
    auto b = std::make_shared<rhmc_ctx::TabBuf>();
    b->s = st;
    if (hipMalloc(&b->p, bytes) != hipSuccess) {
      b->p = nullptr;
      return fail(RHMC_ERR_NOMEM, "hipMalloc of " + std::to_string(bytes) +
                                      " B of windowed factor tables failed");
    }
    b->bytes = bytes;
    if (t)
      t->buf = std::move(b);  // the old buffer goes with its last lease
    else
      ctx->tabs.push_back({st, std::move(b)});
    t = nullptr;
    for (auto& e : ctx->tabs)
      if (e.s == st) t = &e;
  }
  // 0xFF bytes are NaN doubles: a read of an entry this launch did not write
  // turns its chain's result NaN (status NONFINITE) instead of reusing a
  // previous launch's value.
  if (poison) HIP_TRY(hipMemsetAsync(t->buf->p, 0xFF, bytes, st));
  *out = (double*)t->buf->p;
  *lease = t->buf;
  return RHMC_OK;
}

// ---------------------------------------------------------------------------
// Kernel arguments: one builder per struct
// ---------------------------------------------------------------------------

Geometry make_geometry(int rows, int cols) {
  const int npix = rows * cols;
  return Geometry{rows, cols, npix, /*npl*/ (npix + kWave - 1) / kWave, /*di*/ kWave / cols,
                  /*dj*/ kWave % cols, /*work*/ nullptr};
}

int make_consts(const rhmc_params* P, Consts* c) {
  if (!P) return fail(RHMC_ERR_ARG, "params is NULL");
  if (P->reserved != 0) return fail(RHMC_ERR_ARG, "params.reserved must be 0");
  std::memset(c, 0, sizeof(*c));
  c->dt = P->dt;
  c->hdt = P->dt / 2.0;
  c->delta = P->delta;
  c->B = P->B_count;
  c->f_lim = P->f_lim;
  c->f_low = P->f_low;
  const double sigma = P->fwhm_pix / 2.354;  // utils.py:480
  c->two_sig2 = 2 * (sigma * sigma);         // 2*sigma**2 (:484)
  c->psf_norm = (M_PI * 2) * (sigma * sigma);
  const double sv = P->fwhm_pix / 2.354;
  c->var = sv * sv;  // (PSF_FWHM_pix/2.354)**2 (sampler_RHMC.py:384)
  c->g_xx = P->g_xx;
  c->g_ff = P->g_ff;
  c->g_ff2 = P->g_ff2;
  c->g0 = P->g0;
  c->g1 = P->g1;
  c->g2 = P->g2;
  c->c0 = (P->B_count / P->g0) / P->g_ff;
  c->alpha = P->alpha;
  c->beta = P->beta;
  c->vc_pow = P->Vc_r_pow;
  c->vprior = P->V_prior_const;
  c->inv_gff2 = 1.0 / c->g_ff2;
  c->inv_g1 = 1.0 / c->g1;
  c->Bg2 = c->B / c->g2;
  c->two_Bg2 = 2.0 * c->Bg2;
  c->inv_gxx = 1.0 / c->g_xx;
  c->inv_two_sig2 = 1.0 / c->two_sig2;
  c->inv_norm = 1.0 / c->psf_norm;
  c->inv_var = 1.0 / c->var;
  {  // PSF factor recurrences of the register-window kernels (rhmc_tiledr.hpp)
    const double ci = c->inv_two_sig2;
    c->k_row = std::exp(-2.0 * ci);
    c->k_col4 = std::exp(-32.0 * ci);
    // |v0| < rec_vmax keeps every base exp above the fp64 normal range
    // (c v0^2 < 700) and every ratio below e^700 over up to 8 rows (row
    // ratios: c (2 (|v0| + 8) + 1) < 700) or 8 columns 4 apart (column
    // ratios: c (8 (|w0| + 32) + 16) < 700); outside it the direct factors run
    double vm = std::sqrt(700.0 / ci);
    vm = std::fmin(vm, (700.0 / ci - 17.0) / 2.0);
    vm = std::fmin(vm, 700.0 / (8.0 * ci) - 34.0);
    c->rec_vmax = (ci > 0.0 && vm > 0.0) ? vm : 0.0;
  }
  c->near_f = P->f_lim - 0x1p-40 * std::fmax(1.0, std::fabs(P->f_lim));
  c->counter_max = P->counter_max;
  c->use_prior = P->use_prior != 0;
  c->use_Vc = P->use_Vc != 0;
  return RHMC_OK;
}

// One-star kernels (register-window, lane-group); the launcher sets Df.
LeapArgsK1 k1_args(const rhmc_ctx* ctx, const Consts& c, double* q, double* p, int32_t* it,
                   int32_t* st, int64_t n, int n_steps) {
  return LeapArgsK1{q, p, it, st, ctx->d_D, /*Df*/ nullptr, n, n_steps, ctx->rows, ctx->cols,
                    /*pad*/ 0, c};
}

// Multi-star register kernels (pixel-major, register-window); the launcher
// sets Df.  dtv / steps: HMC_random only.
LeapArgsKR kr_args(const rhmc_ctx* ctx, const Consts& c, double* q, double* p, int32_t* it,
                   int32_t* st, int64_t n, int K, int n_steps, const double* dtv = nullptr,
                   const int32_t* steps = nullptr) {
  return LeapArgsKR{q, p, it, st, ctx->d_D, /*Df*/ nullptr, n, K, n_steps, /*side*/ ctx->rows,
                    /*pad*/ 0, c, dtv, steps};
}

// One-wave-per-chain kernels (the slotted frame, the LDS-image step).
LeapArgs leap_args(const rhmc_ctx* ctx, const Consts& c, double* q, double* p, int32_t* it,
                   int32_t* st, int64_t n, int K, int n_steps) {
  return LeapArgs{q, p, it, st, ctx->d_D, n, K, n_steps, make_geometry(ctx->rows, ctx->cols), c};
}

EnergyArgs energy_args(const rhmc_ctx* ctx, const Consts& c, const double* q, const double* p,
                       double* V, double* T, int64_t n, int K, int f_pos) {
  return EnergyArgs{q, p, V, T, ctx->d_D, n, K, f_pos & (RHMC_V_FLUX_WALL | RHMC_V_NO_POSCHECK),
                    make_geometry(ctx->rows, ctx->cols), c};
}

// A ragged set's rows and star counts (LeapArgs, LeapArgsKR, EnergyArgs).
template <class A>
void set_ragged(A& a, const int32_t* d_K, const int64_t* d_rows, int64_t ld) {
  a.Kc = d_K;
  a.rows = d_rows;
  a.ld = ld;
}

// The MH kernels' record pointers (MhArgs, MhK1Args, MhKArgs); rec nullable.
template <class A>
void set_record(A& k, const rhmc_mh_record* rec) {
  k.q_chain = rec ? rec->q_chain : nullptr;
  k.E_chain = rec ? rec->E_chain : nullptr;
  k.V_chain = rec ? rec->V_chain : nullptr;
  k.T_chain = rec ? rec->T_chain : nullptr;
  k.accept = rec ? rec->accept : nullptr;
}

// ---------------------------------------------------------------------------
// Slotted kernels: the launch shape, written once
// ---------------------------------------------------------------------------
struct SlotShape {
  dim3 grid, block;
  size_t lds = 0;
  TableLease lease;  // held until the launch is enqueued
};

// W waves per workgroup and the LDS they need.  LDS-image: W waves share one
// LDS copy of D, the largest W <= 4 whose LDS fits.  Windowed: LDS = W * tables
// (K <= 256: 136 KB for one wave, within gfx950's 160 KB; a device with less
// LDS gets RHMC_ERR_UNSUPPORTED here, not a failed launch); WinGG: the exp
// table only; dense: four waves (32 px: 41.5 KB, 48 px: 92.6 KB).
int pick_waves_slotted(const rhmc_ctx* ctx, const Plan& pl, int K, size_t* lds, int* W) {
  const size_t max_lds = (size_t)ctx->max_lds;
  *W = 4;
  if (pl.family == Family::LdsImage) {  // the bytes do not depend on MAXK
    using L = LdsG<kMaxKGeneric>;
    while (*W > 1 && L::lds_bytes(*W, K, ctx->rows, ctx->cols) > max_lds) *W >>= 1;
    *lds = L::lds_bytes(*W, K, ctx->rows, ctx->cols);
    if (*lds > max_lds)
      return fail(RHMC_ERR_UNSUPPORTED,
                  "image + PSF tables exceed LDS (" + std::to_string(*lds) + " B > " +
                      std::to_string(ctx->max_lds) + " B); large images are not built yet");
    return RHMC_OK;
  }
  switch (pl.policy) {
    case Policy::DenseG:
      *lds = pl.path == 32 ? DenseG<32>::lds_bytes(4) : DenseG<48>::lds_bytes(4);
      if (*lds > max_lds) return fail(RHMC_ERR_UNSUPPORTED, "dense kernel LDS");
      return RHMC_OK;
    case Policy::WinGG:
      *lds = WinGG::lds_bytes(4, K);
      return RHMC_OK;
    case Policy::WinEG:
      while (*W > 1 && WinEG::lds_bytes(*W, K) > max_lds) *W >>= 1;
      *lds = WinEG::lds_bytes(*W, K);
      if (*lds > max_lds)
        return fail(RHMC_ERR_UNSUPPORTED, "windowed energy tables exceed the device's LDS");
      return RHMC_OK;
    case Policy::WinG:
      break;
  }
  while (*W > 1 && WinG::lds_bytes(*W, K) > max_lds) *W >>= 1;
  *lds = WinG::lds_bytes(*W, K);
  if (*lds > max_lds)
    return fail(RHMC_ERR_UNSUPPORTED, "windowed PSF tables for K = " + std::to_string(K) +
                                          " exceed the device's LDS (" + std::to_string(*lds) +
                                          " B > " + std::to_string(ctx->max_lds) + " B)");
  return RHMC_OK;
}

// Workgroup, WinGG's table lease (into g->work) and the grid of one wave per
// chain.  set_device: the callers that have not selected the device yet do it
// between the two, as they always have.
int slotted_shape(const rhmc_ctx* ctx, const Plan& pl, int K, int64_t n, hipStream_t s,
                  bool set_device, Geometry* g, SlotShape* sh) {
  int W;
  if (int rc = pick_waves_slotted(ctx, pl, K, &sh->lds, &W)) return rc;
  if (set_device) HIP_TRY(hipSetDevice(ctx->device));
  if (int rc = work_tables(ctx, pl, K, n, s, &g->work, &sh->lease)) return rc;
  sh->grid = dim3((unsigned)((n + W - 1) / W));
  sh->block = dim3(W * kWave);
  return RHMC_OK;
}

int launch_leap_slotted(const rhmc_ctx* ctx, const Plan& pl, LeapArgs a, hipStream_t s) {
  SlotShape sh;
  if (int rc = slotted_shape(ctx, pl, a.K, a.n_chains, s, false, &a.g, &sh)) return rc;
  return with_policy(pl, [&](auto gt, auto st) {
    using G = typename decltype(gt)::type;
    hipLaunchKernelGGL((leapfrog_win_kernel<G, decltype(st)::value>), sh.grid, sh.block, sh.lds,
                       s, a);
    return launch_status();
  });
}

int launch_energy_slotted(const rhmc_ctx* ctx, const Plan& pl, EnergyArgs a, hipStream_t s) {
  SlotShape sh;
  if (int rc = slotted_shape(ctx, pl, a.K, a.n_chains, s, false, &a.g, &sh)) return rc;
  return with_perwave_energy_policy(pl, [&](auto gt, auto st) {
    using G = typename decltype(gt)::type;
    hipLaunchKernelGGL((energy_win_kernel<G, decltype(st)::value>), sh.grid, sh.block, sh.lds, s,
                       a);
    return launch_status();
  });
}

// ---------------------------------------------------------------------------
// One-star kernels
// ---------------------------------------------------------------------------

// Launch shape of a one-star kernel layout TL (TiledR, TiledL): four waves per
// workgroup, TL::CPW chains per wave, the image in LDS.
template <class TL>
int k1_shape(const rhmc_ctx* ctx, int64_t n, dim3* grid, dim3* block, size_t* lds) {
  *lds = TL::lds_bytes();
  if (*lds > (size_t)ctx->max_lds) return fail(RHMC_ERR_UNSUPPORTED, "image too large for LDS");
  constexpr int W = 4;
  const int64_t waves = (n + TL::CPW - 1) / TL::CPW;
  *grid = dim3((unsigned)((waves + W - 1) / W));
  *block = dim3(W * kWave);
  return RHMC_OK;
}

// Register-window single-star kernel (rhmc_tiledr.hpp).
template <int IMG, int WIN, typename DT, bool PROF>
int launch_tiledr_t(const rhmc_ctx* ctx, const LeapArgsK1& a, hipStream_t s) {
  dim3 grid, block;
  size_t lds;
  if (int rc = k1_shape<TiledR<IMG, WIN, DT>>(ctx, a.n_chains, &grid, &block, &lds)) return rc;
  hipLaunchKernelGGL((leapfrog_k1_tiledr<IMG, WIN, DT, PROF>), grid, block, lds, s, a);
  return launch_status();
}
// The plan's window and pixel cache (fp32 when the image allows it exactly).
// A library built with -DRHMC_PHASE_PROF (make prof, tools/phase_prof.py only)
// runs the phase-timing instantiation of the 28-px fp32 body instead, which
// writes cycle counts over the state.
int launch_tiledr(const rhmc_ctx* ctx, const Plan& pl, LeapArgsK1 a, hipStream_t s) {
  if (pl.f32) a.Df = ctx->d_Df;
  return with_regwin1(pl, ctx->rows, [&](auto img, auto win, auto dt) {
    using DT = typename decltype(dt)::type;
    constexpr int WIN = decltype(win)::value;
#ifdef RHMC_PHASE_PROF
    constexpr bool PROF = WIN == 28 && std::is_same<DT, float>::value;
#else
    constexpr bool PROF = false;
#endif
    return launch_tiledr_t<decltype(img)::value, WIN, DT, PROF>(ctx, a, s);
  });
}

// Lane-group single-star kernel for large batches (rhmc_tiledl.hpp).
template <int IMG, typename DT, int LPC>
int launch_tiledl_t(const rhmc_ctx* ctx, const LeapArgsK1& a, hipStream_t s) {
  dim3 grid, block;
  size_t lds;
  if (int rc = k1_shape<TiledL<IMG, 28, DT, LPC>>(ctx, a.n_chains, &grid, &block, &lds))
    return rc;
  hipLaunchKernelGGL((leapfrog_k1_tiledl<IMG, 28, DT, LPC>), grid, block, lds, s, a);
  return launch_status();
}
int launch_tiledl(const rhmc_ctx* ctx, const Plan& pl, LeapArgsK1 a, hipStream_t s) {
  if (pl.f32) a.Df = ctx->d_Df;
  return with_lane(pl, ctx->rows, [&](auto img, auto dt, auto lpc) {
    using DT = typename decltype(dt)::type;
    return launch_tiledl_t<decltype(img)::value, DT, decltype(lpc)::value>(ctx, a, s);
  });
}

// The other one-star register-window kernels (explicit integrators,
// HMC_random, energy, fused MH, find_peaks): 28-px window on a 32/48/64-px
// image.  go(IntTag<IMG>, TypeTag<DT>, grid, block, lds) enqueues the kernel;
// the caller has set Df.
template <class F>
int launch_k1_w28(const rhmc_ctx* ctx, const Plan& pl, int64_t n, F&& go) {
  return with_k1_w28(pl, ctx->rows, [&](auto img, auto dt) {
    using TL = TiledR<decltype(img)::value, 28, typename decltype(dt)::type>;
    dim3 grid, block;
    size_t lds;
    if (int rc = k1_shape<TL>(ctx, n, &grid, &block, &lds)) return rc;
    go(img, dt, grid, block, lds);
    return launch_status();
  });
}

// ---------------------------------------------------------------------------
// Multi-star register kernels
// ---------------------------------------------------------------------------

// Multi-star register-window kernel (rhmc_tiledrk.hpp): K in [1, 64], square
// image of side >= 32, PSF narrow enough for the 28-row window.
template <typename DT, int SLOTS, bool TAB, int SOLVER, int WS>
int launch_kr_ws(const rhmc_ctx* ctx, const LeapArgsKR& a, int f_pos, hipStream_t s) {
  using TK = TiledRK<DT, SLOTS, TAB>;
  int W = 4;
  while (W > WS && TK::lds_bytes(W, a.K, a.side, WS) > (size_t)ctx->max_lds / 2) W >>= 1;
  const size_t lds = TK::lds_bytes(W, a.K, a.side, WS);
  if (lds > (size_t)ctx->max_lds) return fail(RHMC_ERR_UNSUPPORTED, "factor tables exceed LDS");
  const int64_t waves = (a.n_chains + TK::CPW - 1) / TK::CPW * WS;
  const dim3 grid((unsigned)((waves + W - 1) / W)), block(W * kWave);
  hipLaunchKernelGGL((leapfrog_kr<DT, SLOTS, TAB, SOLVER, WS>), grid, block, lds, s, a, f_pos);
  return launch_status();
}

template <int SOLVER = RHMC_SOLVER_IMPLICIT>
int launch_kr(const rhmc_ctx* ctx, const Plan& pl, LeapArgsKR a, int f_pos, hipStream_t s) {
  if (pl.f32) a.Df = ctx->d_Df;
  return with_multiwin<SOLVER == RHMC_SOLVER_IMPLICIT>(
      pl, [&](auto dt, auto slots, auto tab, auto ws) {
        using DT = typename decltype(dt)::type;
        return launch_kr_ws<DT, decltype(slots)::value, decltype(tab)::value, SOLVER,
                            decltype(ws)::value>(ctx, a, f_pos, s);
      });
}

// Pixel-major multi-star kernel (rhmc_pixk.hpp), 32/48-px fp32-exact images.
template <int IMG, int SOLVER = RHMC_SOLVER_IMPLICIT, bool RAGGED = false>
int launch_pk(const rhmc_ctx* ctx, LeapArgsKR a, hipStream_t s, int f_pos = 0) {
  using PK = PixK<IMG, 10>;  // LDS layout does not depend on the columns per pass
  int W = 4;
  while (W > 1 && PK::lds_bytes(W) > (size_t)ctx->max_lds / 2) W >>= 1;
  const size_t lds = PK::lds_bytes(W);
  if (lds > (size_t)ctx->max_lds) return fail(RHMC_ERR_UNSUPPORTED, "pixk LDS");
  a.Df = ctx->d_Df;
  const int64_t waves = (a.n_chains + PK::CPW - 1) / PK::CPW;
  const dim3 grid((unsigned)((waves + W - 1) / W)), block(W * kWave);
  hipLaunchKernelGGL((leapfrog_pk<IMG, 10, SOLVER, RAGGED>), grid, block, lds, s, a, f_pos);
  return launch_status();
}

// The multi-star plan (pixel-major or register-window) with integrator SOLVER.
template <int SOLVER>
int launch_multi(const rhmc_ctx* ctx, const Plan& pl, const LeapArgsKR& a, int f_pos,
                 hipStream_t s) {
  if (pl.family == Family::PixMajor)
    return with_side2(ctx->rows, [&](auto img) {
      return launch_pk<decltype(img)::value, SOLVER>(ctx, a, s, f_pos);
    });
  return launch_kr<SOLVER>(ctx, pl, a, f_pos, s);
}

// ---------------------------------------------------------------------------
// The operations
// ---------------------------------------------------------------------------

// n_steps implicit steps of n_chains chains on device buffers, async on `s`.
int launch_leapfrog(rhmc_ctx* ctx, const rhmc_params* P, double* d_q, double* d_p,
                    int64_t n_chains, int32_t K, int32_t n_steps, int32_t* d_it, int32_t* d_st,
                    hipStream_t s) {
  Consts c;
  int rc = make_consts(P, &c);
  if (rc) return rc;
  if (n_steps < 0) return fail(RHMC_ERR_ARG, "n_steps < 0");
  if (P->counter_max < 1) return fail(RHMC_ERR_ARG, "counter_max < 1");
  if (n_chains == 0) return RHMC_OK;
  HIP_TRY(hipSetDevice(ctx->device));
  Plan pl;
  if ((rc = plan_for(ctx, c, Op::Step, K, n_chains, &pl))) return rc;
  switch (pl.family) {
    case Family::RegWin1: {
      const LeapArgsK1 t = k1_args(ctx, c, d_q, d_p, d_it, d_st, n_chains, n_steps);
      return launch_tiledr(ctx, pl, t, s);
    }
    case Family::Lane: {
      const LeapArgsK1 t = k1_args(ctx, c, d_q, d_p, d_it, d_st, n_chains, n_steps);
      return launch_tiledl(ctx, pl, t, s);
    }
    case Family::PixMajor:
    case Family::MultiWin:
      return launch_multi<RHMC_SOLVER_IMPLICIT>(
          ctx, pl, kr_args(ctx, c, d_q, d_p, d_it, d_st, n_chains, K, n_steps), 0, s);
    case Family::Slotted:
      return launch_leap_slotted(ctx, pl,
                                 leap_args(ctx, c, d_q, d_p, d_it, d_st, n_chains, K, n_steps), s);
    default: {  // LDS-image: leapfrog_kernel<MAXK>, the frame's launch shape
      LeapArgs a = leap_args(ctx, c, d_q, d_p, d_it, d_st, n_chains, K, n_steps);
      SlotShape sh;
      if ((rc = slotted_shape(ctx, pl, K, n_chains, s, false, &a.g, &sh))) return rc;
      return with_maxk(pl, [&](auto mk) {
        hipLaunchKernelGGL(leapfrog_kernel<decltype(mk)::value>, sh.grid, sh.block, sh.lds, s, a);
        return launch_status();
      });
    }
  }
}

// V (and optionally T) of n chains on device buffers, async on `s`.
int launch_energy(const rhmc_ctx* ctx, const Consts& c, const double* d_q, const double* d_p,
                  double* d_V, double* d_T, int64_t n, int K, int f_pos, hipStream_t s) {
  Plan pl;
  if (int rc = plan_for(ctx, c, Op::Energy, K, n, &pl)) return rc;
  const EnergyArgs a = energy_args(ctx, c, d_q, d_p, d_V, d_T, n, K, f_pos);
  switch (pl.family) {
    case Family::RegWin1: {  // rhmc_mhk1.hpp
      if (n == 0) return RHMC_OK;
      const EnergyK1Args k{d_q, d_p, d_V, d_T, ctx->d_D, pl.f32 ? ctx->d_Df : nullptr, n, a.f_pos,
                           /*pad*/ 0, c};
      return launch_k1_w28(ctx, pl, n,
                           [&](auto img, auto dt, dim3 grid, dim3 block, size_t lds) {
        using DT = typename decltype(dt)::type;
        hipLaunchKernelGGL((energy_k1_tiledr<decltype(img)::value, DT>), grid, block, lds, s, k);
      });
    }
    default: return launch_energy_slotted(ctx, pl, a, s);  // slotted, LDS-image
  }
}

// dVdq (kind 0) or dphidq (kind 1) of n chains on device buffers, async on `s`.
int launch_gradient(const rhmc_ctx* ctx, const Plan& pl, const Consts& c, const double* d_q,
                    double* d_grad, int64_t n, int K, int kind, hipStream_t s) {
  GradArgs a{d_q, d_grad, ctx->d_D, n, K, /*with_metric*/ kind,
             make_geometry(ctx->rows, ctx->cols), c};
  SlotShape sh;
  if (int rc = slotted_shape(ctx, pl, K, n, s, false, &a.g, &sh)) return rc;
  return with_perwave_policy(pl, [&](auto gt, auto st) {
    using G = typename decltype(gt)::type;
    hipLaunchKernelGGL((gradient_win_kernel<G, decltype(st)::value>), sh.grid, sh.block, sh.lds,
                       s, a);
    return launch_status();
  });
}

// [K_min, K_max]: one ragged family (rhmc_select.hpp) and one register-slot
// count (the launch's SLOTS and LDS follow K_max)
int ragged_check(const rhmc_ctx* ctx, const Consts& c, int K_min, int K_max, int64_t ld) {
  if (K_min < 1 || K_max > kMaxK || K_min > K_max)
    return fail(RHMC_ERR_ARG, "ragged set: need 1 <= K_min <= K_max <= 1024");
  if (win_slots(K_min) != win_slots(K_max))
    return fail(RHMC_ERR_ARG, "ragged set: K_min and K_max need the same register slots "
                              "(1-64, 65-128, 129-256, 257-512, 513-1024 stars)");
  if (ld < 3 * (int64_t)K_max) return fail(RHMC_ERR_ARG, "ragged set: ld < 3 K_max");
  const SelectIn in = select_in(ctx);
  const int f = ragged_family(in, c.use_Vc, c.inv_two_sig2, K_min);
  for (int K = K_min; K <= K_max; ++K)
    if (ragged_family(in, c.use_Vc, c.inv_two_sig2, K) != f || f == 0)
      return fail(RHMC_ERR_UNSUPPORTED, "ragged set: K = " + std::to_string(K) +
                                            " is not served by a slotted kernel on this image "
                                            "(rhmc_ragged_ok)");
  return RHMC_OK;
}

// The step on a ragged set: K_max's plan, which ragged_check has made the
// plan of every K of the set.
int launch_leapfrog_ragged(rhmc_ctx* ctx, const rhmc_params* P, double* d_q, double* d_p,
                           int64_t ld, const int64_t* d_rows, const int32_t* d_K, int64_t n,
                           int K_min, int K_max, int32_t n_steps, hipStream_t s) {
  Consts c;
  int rc = make_consts(P, &c);
  if (rc) return rc;
  if (n_steps < 0) return fail(RHMC_ERR_ARG, "n_steps < 0");
  if (P->counter_max < 1) return fail(RHMC_ERR_ARG, "counter_max < 1");
  if ((rc = ragged_check(ctx, c, K_min, K_max, ld))) return rc;
  if (n == 0) return RHMC_OK;
  HIP_TRY(hipSetDevice(ctx->device));
  Plan pl;
  if ((rc = plan_for(ctx, c, Op::Step, K_max, n, &pl))) return rc;
  if (pl.family == Family::PixMajor) {  // each chain its own row and K
    LeapArgsKR t = kr_args(ctx, c, d_q, d_p, nullptr, nullptr, n, K_max, n_steps);
    set_ragged(t, d_K, d_rows, ld);
    return with_side2(ctx->rows, [&](auto img) {
      return launch_pk<decltype(img)::value, RHMC_SOLVER_IMPLICIT, true>(ctx, t, s);
    });
  }
  LeapArgs a = leap_args(ctx, c, d_q, d_p, nullptr, nullptr, n, K_max, n_steps);
  set_ragged(a, d_K, d_rows, ld);
  return launch_leap_slotted(ctx, pl, a, s);
}

int launch_energy_ragged(rhmc_ctx* ctx, const rhmc_params* P, const double* d_q, int64_t ld,
                         const int64_t* d_rows, const int32_t* d_K, int64_t n, int K_min,
                         int K_max, int f_pos, double* d_V, hipStream_t s) {
  Consts c;
  int rc = make_consts(P, &c);
  if (rc) return rc;
  if ((rc = ragged_check(ctx, c, K_min, K_max, ld))) return rc;
  if (n == 0) return RHMC_OK;
  HIP_TRY(hipSetDevice(ctx->device));
  Plan pl;
  if ((rc = plan_for(ctx, c, Op::Energy, K_max, n, &pl))) return rc;
  EnergyArgs a = energy_args(ctx, c, d_q, nullptr, d_V, nullptr, n, K_max, f_pos);
  set_ragged(a, d_K, d_rows, ld);
  return launch_energy_slotted(ctx, pl, a, s);  // LDS-image: the pixel-major step's energy
}

// ---------------------------------------------------------------------------
// Metropolis-Hastings
// ---------------------------------------------------------------------------

// The run's parameters at MH iteration l: multi_gym.run_RHMC's schedules
// (sampler_RHMC.py:1010-1016) set g_ff2 = schedule_g_ff2[l] and beta =
// schedule_beta[l] while l < the schedule's size and keep the last value
// after it; no schedule keeps P's value.
rhmc_params sched_params(const rhmc_params& P, const rhmc_mh_schedule* sc, int l) {
  rhmc_params q = P;
  if (sc && sc->g_ff2 && sc->n_g_ff2 > 0) q.g_ff2 = sc->g_ff2[l < sc->n_g_ff2 ? l : sc->n_g_ff2 - 1];
  if (sc && sc->beta && sc->n_beta > 0) q.beta = sc->beta[l < sc->n_beta ? l : sc->n_beta - 1];
  return q;
}

bool sched_active(const rhmc_mh_schedule* sc) {
  return sc && ((sc->g_ff2 && sc->n_g_ff2 > 0) || (sc->beta && sc->n_beta > 0));
}

// One star: the whole MH loop in one launch (rhmc_mhk1.hpp).
int launch_mh_k1(const rhmc_ctx* ctx, const Plan& pl, MhK1Args k, hipStream_t s) {
  if (pl.f32) k.Df = ctx->d_Df;
  return launch_k1_w28(ctx, pl, k.n, [&](auto img, auto dt, dim3 grid, dim3 block, size_t lds) {
    using DT = typename decltype(dt)::type;
    hipLaunchKernelGGL((mh_k1_tiledr<decltype(img)::value, 28, DT>), grid, block, lds, s, k);
  });
}

// V(q) once, then one mh_pk_iter launch per iteration (rhmc_mhpk.hpp); V
// [n] is the carried V(q) (device scratch).  A schedule changes only g_ff2
// and beta, which this kernel's V does not read (no repulsion here), so the
// carried V stays exact; each launch gets its iteration's constants.
template <int IMG>
int launch_mh_pk(const rhmc_ctx* ctx, MhKArgs k, double* V, hipStream_t s,
                 const rhmc_params* P, const rhmc_mh_schedule* sc) {
  using MP = MhPK<IMG, 10>;
  int W = 4;
  while (W > 1 && MP::lds_bytes(W) > (size_t)ctx->max_lds / 2) W >>= 1;
  const size_t lds = MP::lds_bytes(W);
  if (lds > (size_t)ctx->max_lds) return fail(RHMC_ERR_UNSUPPORTED, "mh_pk LDS");
  k.Df = ctx->d_Df;
  const int64_t waves = (k.n + MP::PK::CPW - 1) / MP::PK::CPW;
  const dim3 grid((unsigned)((waves + W - 1) / W)), block(W * kWave);
  hipLaunchKernelGGL((mh_pk_v0<IMG, 10>), grid, block, lds, s, k, V);
  HIP_TRY(hipGetLastError());
  for (int it = 0; it < k.n_iter; ++it) {
    if (sched_active(sc)) {
      const rhmc_params Pl = sched_params(*P, sc, it);
      int rc = make_consts(&Pl, &k.c);
      if (rc) return rc;
    }
    hipLaunchKernelGGL((mh_pk_iter<IMG, 10>), grid, block, lds, s, k, it, V);
    HIP_TRY(hipGetLastError());
  }
  return RHMC_OK;
}

// The four-kernel loop's begin (END = false) or end of one MH iteration.
template <bool END>
int launch_mh_turn(const MhArgs& m, hipStream_t s) {
  return with_mh_wave(mh_wave(m.K), [&](auto wave) {
    constexpr bool WAVE = decltype(wave)::value;
    const dim3 grid((unsigned)(WAVE ? (m.n + 3) / 4 : (m.n + 255) / 256)), block(256);
    if constexpr (WAVE && END) hipLaunchKernelGGL(mh_end_wave_kernel, grid, block, 0, s, m);
    else if constexpr (WAVE) hipLaunchKernelGGL(mh_begin_wave_kernel, grid, block, 0, s, m);
    else if constexpr (END) hipLaunchKernelGGL(mh_end_kernel, grid, block, 0, s, m);
    else hipLaunchKernelGGL(mh_begin_kernel, grid, block, 0, s, m);
    return launch_status();
  });
}

// The MH outer loop on device buffers (sampler_RHMC.py:1018-1083): per
// iteration begin -> n_steps fused leapfrog -> V(q') -> accept, all queued on
// `s` with no host synchronisation.  `rec` holds device pointers (nullable);
// `sc` (nullable, host arrays) schedules g_ff2 / beta per iteration
// (sampler_RHMC.py:1010-1016, sched_params).
int run_mh(rhmc_ctx* ctx, const rhmc_params* P, double* d_q, int64_t n, int32_t K,
           int32_t n_iter, int32_t n_steps, int32_t f_pos, const double* d_z, const double* d_u,
           uint64_t seed, const rhmc_mh_record* rec, hipStream_t s,
           const rhmc_mh_schedule* sc = nullptr) {
  Consts c;
  int rc = make_consts(P, &c);
  if (rc) return rc;
  if (n_iter < 0 || n_steps < 0) return fail(RHMC_ERR_ARG, "n_iter/n_steps < 0");
  if (sc && (sc->n_g_ff2 < 0 || sc->n_beta < 0 || (sc->n_g_ff2 > 0 && !sc->g_ff2) ||
             (sc->n_beta > 0 && !sc->beta)))
    return fail(RHMC_ERR_ARG, "schedule: negative size or NULL array with a nonzero size");
  const bool sched = sched_active(sc);
  if (sched)  // every iteration's parameters must be valid, not only the first's
    for (int it = 0; it < n_iter; ++it) {
      const rhmc_params Pl = sched_params(*P, sc, it);
      Consts cl;
      if ((rc = make_consts(&Pl, &cl))) return rc;
    }
  if (n == 0 || n_iter == 0) return RHMC_OK;
  f_pos = f_pos != 0 ? RHMC_V_FLUX_WALL : 0;
  Plan fused;
  if ((rc = plan_for(ctx, c, Op::MhFused, K, n, &fused))) return rc;
  if (fused.family == Family::RegWin1) {
    MhK1Args k;
    k.q = d_q;
    k.D = ctx->d_D;
    k.Df = nullptr;
    k.z = d_z;
    k.u = d_u;
    set_record(k, rec);
    k.n = n;
    k.n_iter = n_iter;
    k.n_steps = n_steps;
    k.f_pos = f_pos;
    k.it0 = 0;
    k.seed = seed;
    k.c = c;
    if (!sched) return launch_mh_k1(ctx, fused, k, s);
    // scheduled: one launch per iteration with its own constants (V(q) is
    // re-evaluated at each launch's start: the same operations, the same value)
    for (int it = 0; it < n_iter; ++it) {
      const rhmc_params Pl = sched_params(*P, sc, it);
      if ((rc = make_consts(&Pl, &k.c))) return rc;
      k.n_iter = 1;
      k.it0 = it;
      if ((rc = launch_mh_k1(ctx, fused, k, s))) return rc;
    }
    return RHMC_OK;
  }
  if (fused.family == Family::PixMajor) {
    MhKArgs k;
    k.q = d_q;
    k.Df = nullptr;
    k.z = d_z;
    k.u = d_u;
    set_record(k, rec);
    k.n = n;
    k.K = K;
    k.n_iter = n_iter;
    k.n_steps = n_steps;
    k.f_pos = f_pos;
    k.seed = seed;
    k.c = c;
    if ((rc = ensure_mh_scratch(ctx, (size_t)n * sizeof(double) + 256))) return rc;
    double* V = (double*)ctx->mh_scratch;
    return with_side2(ctx->rows, [&](auto img) {
      return launch_mh_pk<decltype(img)::value>(ctx, k, V, s, P, sc);
    });
  }
  const size_t sb = (size_t)n * 3 * K * sizeof(double), eb = (size_t)n * sizeof(double);
  if ((rc = ensure_mh_scratch(ctx, 2 * sb + 3 * eb + 256))) return rc;
  char* b = (char*)ctx->mh_scratch;
  MhArgs m;
  m.q = d_q;
  m.q_prop = (double*)b;
  m.p = (double*)(b + sb);
  m.V_cur = (double*)(b + 2 * sb);
  m.V_prop = (double*)(b + 2 * sb + eb);
  m.E0 = (double*)(b + 2 * sb + 2 * eb);
  m.z = d_z;
  m.u = d_u;
  set_record(m, rec);
  m.n = n;
  m.K = K;
  m.seed = seed;
  m.c = c;
  if ((rc = launch_energy(ctx, c, d_q, nullptr, m.V_cur, nullptr, n, K, f_pos, s))) return rc;
  // V reads beta through the repulsion term: a beta schedule re-evaluates
  // V(q) at each iteration's start, like the reference's V_initial (:1025)
  const bool v_sched = sched && c.use_Vc && sc->beta && sc->n_beta > 0;
  for (int it = 0; it < n_iter; ++it) {
    m.iter = it;
    const rhmc_params Pl = sched ? sched_params(*P, sc, it) : *P;
    if (sched) {
      if ((rc = make_consts(&Pl, &m.c))) return rc;
      if (v_sched &&
          (rc = launch_energy(ctx, m.c, d_q, nullptr, m.V_cur, nullptr, n, K, f_pos, s)))
        return rc;
    }
    if ((rc = launch_mh_turn<false>(m, s))) return rc;
    if ((rc = launch_leapfrog(ctx, &Pl, m.q_prop, m.p, n, K, n_steps, nullptr, nullptr, s)))
      return rc;
    if ((rc = launch_energy(ctx, m.c, m.q_prop, nullptr, m.V_prop, nullptr, n, K, f_pos, s)))
      return rc;
    if ((rc = launch_mh_turn<true>(m, s))) return rc;
  }
  return RHMC_OK;
}

// ---------------------------------------------------------------------------
// Explicit integrators and HMC_random
// ---------------------------------------------------------------------------

int launch_integrate(rhmc_ctx* ctx, const rhmc_params* P, int32_t solver, double* d_q,
                     double* d_p, int64_t n, int32_t K, int32_t n_steps, int32_t f_pos,
                     int32_t* d_st, hipStream_t s) {
  if (solver == RHMC_SOLVER_IMPLICIT)
    return launch_leapfrog(ctx, P, d_q, d_p, n, K, n_steps, nullptr, d_st, s);
  if (solver < RHMC_SOLVER_HMC || solver > RHMC_SOLVER_RHMC_LEAPFROG)
    return fail(RHMC_ERR_ARG, "unknown solver");
  Consts c;
  int rc = make_consts(P, &c);
  if (rc) return rc;
  if (n_steps < 0) return fail(RHMC_ERR_ARG, "n_steps < 0");
  if (n == 0) return RHMC_OK;
  Plan pl;
  if ((rc = plan_for(ctx, c, Op::Integrate, K, n, &pl))) return rc;
  const int fp = f_pos != 0;
  switch (pl.family) {
    case Family::RegWin1: {  // rhmc_tiledr.hpp
      LeapArgsK1 t = k1_args(ctx, c, d_q, d_p, nullptr, d_st, n, n_steps);
      if (pl.f32) t.Df = ctx->d_Df;
      HIP_TRY(hipSetDevice(ctx->device));
      return with_solver(solver, [&](auto sv) {
        return launch_k1_w28(ctx, pl, n,
                             [&](auto img, auto dt, dim3 grid, dim3 block, size_t lds) {
          using DT = typename decltype(dt)::type;
          hipLaunchKernelGGL(
              (integrate_k1_tiledr<decltype(img)::value, 28, DT, decltype(sv)::value>), grid,
              block, lds, s, t, fp);
        });
      });
    }
    case Family::PixMajor:
    case Family::MultiWin: {
      const LeapArgsKR t = kr_args(ctx, c, d_q, d_p, nullptr, d_st, n, K, n_steps);
      HIP_TRY(hipSetDevice(ctx->device));
      return with_solver(solver, [&](auto sv) {
        return launch_multi<decltype(sv)::value>(ctx, pl, t, fp, s);
      });
    }
    default: {  // slotted (integrate_win_kernel)
      LeapArgs a = leap_args(ctx, c, d_q, d_p, nullptr, d_st, n, K, n_steps);
      SlotShape sh;
      if ((rc = slotted_shape(ctx, pl, K, n, s, true, &a.g, &sh))) return rc;
      return with_solver(solver, [&](auto sv) {
        return with_policy(pl, [&](auto gt, auto st) {
          using G = typename decltype(gt)::type;
          hipLaunchKernelGGL((integrate_win_kernel<G, decltype(sv)::value, decltype(st)::value>),
                             sh.grid, sh.block, sh.lds, s, a, fp);
          return launch_status();
        });
      });
    }
  }
}

// HMC_random's trajectories, or with `dg` (device pointers in it)
// RHMC_random_diag's: the same plan and launch shapes, the kernels' DIAG
// bodies, d_dt unused.
template <bool DIAG>
int launch_hmc_random_t(rhmc_ctx* ctx, const Consts& c, const double* d_dt, double* d_q,
                        double* d_p, const int32_t* d_steps, int64_t n, int32_t K, int32_t* d_st,
                        hipStream_t s, const DiagArgs& dg) {
  int rc;
  Plan pl;
  if ((rc = plan_for(ctx, c, Op::HmcRandom, K, n, &pl))) return rc;
  switch (pl.family) {
    case Family::RegWin1: {
      LeapArgsK1 t = k1_args(ctx, c, d_q, d_p, nullptr, d_st, n, 0);
      if (pl.f32) t.Df = ctx->d_Df;
      HIP_TRY(hipSetDevice(ctx->device));
      return launch_k1_w28(ctx, pl, n,
                           [&](auto img, auto dt, dim3 grid, dim3 block, size_t lds) {
        using DT = typename decltype(dt)::type;
        if constexpr (DIAG)
          hipLaunchKernelGGL((diag_hmc_random_k1_tiledr<decltype(img)::value, DT>), grid, block,
                             lds, s, t, d_steps, dg);
        else
          hipLaunchKernelGGL((hmc_random_k1_tiledr<decltype(img)::value, DT>), grid, block, lds,
                             s, t, d_dt, d_steps);
      });
    }
    case Family::PixMajor:
    case Family::MultiWin: {
      LeapArgsKR t = kr_args(ctx, c, d_q, d_p, nullptr, d_st, n, K, 0, d_dt, d_steps);
      t.diag = dg;
      HIP_TRY(hipSetDevice(ctx->device));
      return launch_multi<DIAG ? kSolverDiagRandom : kSolverHmcRandom>(ctx, pl, t, 0, s);
    }
    default: {  // slotted (hmc_random_win_kernel)
      LeapArgs a = leap_args(ctx, c, d_q, d_p, nullptr, d_st, n, K, 0);
      SlotShape sh;
      if ((rc = slotted_shape(ctx, pl, K, n, s, true, &a.g, &sh))) return rc;
      return with_policy(pl, [&](auto gt, auto st) {
        using G = typename decltype(gt)::type;
        if constexpr (DIAG)
          hipLaunchKernelGGL((diag_hmc_random_win_kernel<G, decltype(st)::value>), sh.grid,
                             sh.block, sh.lds, s, a, d_steps, dg);
        else
          hipLaunchKernelGGL((hmc_random_win_kernel<G, decltype(st)::value>), sh.grid, sh.block,
                             sh.lds, s, a, d_dt, d_steps);
        return launch_status();
      });
    }
  }
}

int launch_hmc_random(rhmc_ctx* ctx, const rhmc_params* P, const double* d_dt, double* d_q,
                      double* d_p, const int32_t* d_steps, int64_t n, int32_t K, int32_t* d_st,
                      hipStream_t s) {
  Consts c;
  int rc = make_consts(P, &c);
  if (rc) return rc;
  if (n == 0) return RHMC_OK;
  if (!d_dt || !d_steps) return fail(RHMC_ERR_ARG, "dt/steps is NULL");
  return launch_hmc_random_t<false>(ctx, c, d_dt, d_q, d_p, d_steps, n, K, d_st, s, DiagArgs{});
}

// RHMC_random_diag's trajectories (rhmc_diag_random; check_diag has passed).
// d_trace: nullable [n][o->trace_rows][3K].
int launch_diag_random(rhmc_ctx* ctx, const rhmc_params* P, const rhmc_diag_opts* o, double* d_q,
                       double* d_p, const int32_t* d_steps, int64_t n, int32_t K, int32_t* d_st,
                       double* d_trace, hipStream_t s) {
  Consts c;
  int rc = make_consts(P, &c);
  if (rc) return rc;
  DiagArgs dg;
  dg.dt = o->dt;
  dg.inv_f1 = 1.0 / o->factor1;
  dg.trace = d_trace;
  dg.rows = d_trace ? o->trace_rows : 0;
  return launch_hmc_random_t<true>(ctx, c, nullptr, d_q, d_p, d_steps, n, K, d_st, s, dg);
}

// ---------------------------------------------------------------------------
// HMC_random's / RHMC_random_diag's whole chain (rhmc_chain.hpp)
// ---------------------------------------------------------------------------

// The arguments both entry points share; the record's members may be NULL.
struct ChainCall {
  const double* dt;
  double* q;
  int64_t n;
  int32_t K;
  const double* z;
  const int32_t* steps;
  const double* lnu;
  uint64_t seed;
  const uint64_t* stream_id;
  rhmc_chain_record rec;
};

template <bool DIAG>
int launch_chain_turn(const ChainArgs& a, hipStream_t s) {
  // thread or wave per chain like run_mh's begin / end (launch_mh_turn)
  return with_mh_wave(mh_wave(a.K), [&](auto wave) {
    constexpr bool WAVE = decltype(wave)::value;
    const dim3 grid((unsigned)(WAVE ? (a.n + 3) / 4 : (a.n + 255) / 256)), block(256);
    hipLaunchKernelGGL((chain_turn_kernel<WAVE, DIAG>), grid, block, 0, s, a);
    return launch_status();
  });
}

// The MH loop of samplers.py:504-568 / :722-815 on device buffers
// (check_chain has passed): V(q) once, then per iteration turn -> trajectory
// -> V(q'), and one last turn, all queued on `s` with no host synchronisation.
template <bool DIAG>
int run_chain(rhmc_ctx* ctx, const rhmc_params* P, const rhmc_chain_opts* o, const ChainCall& k,
              hipStream_t s) {
  Consts c;
  int rc = make_consts(P, &c);
  if (rc) return rc;
  HIP_TRY(hipSetDevice(ctx->device));
  const int64_t n = k.n;
  const int K = k.K;
  const size_t sb = ((size_t)n * 3 * K * sizeof(double) + 255) & ~(size_t)255;
  const size_t eb = ((size_t)n * sizeof(double) + 255) & ~(size_t)255;
  if ((rc = ensure_mh_scratch(ctx, 2 * sb + 4 * eb + 256))) return rc;
  char* b = (char*)ctx->mh_scratch;
  ChainArgs a;
  a.q = k.q;
  a.q_prop = (double*)b;
  a.p = (double*)(b + sb);
  a.V_cur = (double*)(b + 2 * sb);
  a.V_prop = (double*)(b + 2 * sb + eb);
  a.E0 = (double*)(b + 2 * sb + 2 * eb);
  a.steps = (int32_t*)(b + 2 * sb + 3 * eb);
  a.z = k.z;
  a.h_steps = k.steps;
  a.lnu = k.lnu;
  a.stream_id = k.stream_id;
  a.q_chain = k.rec.q_chain;
  a.E_chain = k.rec.E_chain;
  a.dE_chain = k.rec.dE_chain;
  a.accept = k.rec.accept;
  a.r_z = k.rec.z;
  a.r_steps = k.rec.steps;
  a.r_lnu = k.rec.lnu;
  a.n = n;
  a.seed = k.seed;
  a.factor1 = o->factor1;
  a.f_lim = P->f_lim;
  a.K = K;
  a.iter = 0;
  a.n_iter = o->n_iter;
  a.iter0 = o->iter0;
  a.steps_min = o->steps_min;
  a.steps_max = o->steps_max;
  DiagArgs dg;
  if (DIAG) {
    dg.dt = o->dt_global;
    dg.inv_f1 = 1.0 / o->factor1;
  }
  const int f_pos = RHMC_V_NO_POSCHECK;            // lightsource_gym.V has no support check
  if ((rc = launch_energy(ctx, c, k.q, nullptr, a.V_cur, nullptr, n, K, f_pos, s))) return rc;
  for (int i = 0;; ++i) {
    a.iter = i;
    if ((rc = launch_chain_turn<DIAG>(a, s))) return rc;
    if (i == o->n_iter) break;
    const int32_t* steps = k.steps ? k.steps + (int64_t)i * n : a.steps;
    int32_t* st = k.rec.status ? k.rec.status + (int64_t)i * n : nullptr;
    if ((rc = launch_hmc_random_t<DIAG>(ctx, c, k.dt, a.q_prop, a.p, steps, n, K, st, s, dg)))
      return rc;
    if ((rc = launch_energy(ctx, c, a.q_prop, nullptr, a.V_prop, nullptr, n, K, f_pos, s)))
      return rc;
  }
  return RHMC_OK;
}

// RHMC_random's kernels (rhmc_hess.hpp; the entry points' checks have passed):
// the trajectory with `o`, else the derivative sets at d_q.  One wave per
// chain, select_hess()'s waves per workgroup and LDS bytes.
int launch_hess(rhmc_ctx* ctx, const rhmc_params* P, const rhmc_hess_opts* o, double* d_q,
                double* d_p, const int32_t* d_steps, int64_t n, int32_t K, int32_t* d_st,
                int32_t* d_done, double* d_dVdq, double* d_dVdqq, double* d_dVdqqq, double* d_V,
                hipStream_t s) {
  HessArgs a;
  int rc = make_consts(P, &a.c);
  if (rc) return rc;
  const HessPlan pl = select_hess(select_in(ctx), K);
  if (pl.message) return fail(RHMC_ERR_UNSUPPORTED, pl.message);
  const int64_t blocks = (n + pl.waves - 1) / pl.waves;
  if (blocks > 0x7fffffff) return fail(RHMC_ERR_UNSUPPORTED, "n_chains exceeds one launch's grid");
  a.q = d_q;
  a.p = d_p;
  a.steps = d_steps;
  a.status = d_st;
  a.steps_done = d_done;
  a.dVdq = d_dVdq;
  a.dVdqq = d_dVdqq;
  a.dVdqqq = d_dVdqqq;
  a.V = d_V;
  a.D = ctx->d_D;
  a.n_chains = n;
  a.K = K;
  a.dt_f = o ? o->dt_f : 0.0;
  a.dt_xy = o ? o->dt_xy : 0.0;
  a.g = make_geometry(ctx->rows, ctx->cols);
  HIP_TRY(hipSetDevice(ctx->device));
  const dim3 grid((unsigned)blocks), block(pl.waves * kWave);
  if (o) hipLaunchKernelGGL(hess_random_kernel, grid, block, pl.lds_bytes, s, a);
  else hipLaunchKernelGGL(hess_derivs_kernel, grid, block, pl.lds_bytes, s, a);
  return launch_status();
}

// ---------------------------------------------------------------------------
// find_peaks' seed descent (rhmc_peaks.hpp)
// ---------------------------------------------------------------------------

int ensure_pin(rhmc_ctx* ctx) {
  if (ctx->h_pin) return RHMC_OK;
  if (hipHostMalloc((void**)&ctx->h_pin, 64, hipHostMallocDefault) != hipSuccess) {
    ctx->h_pin = nullptr;
    return fail(RHMC_ERR_NOMEM, "hipHostMalloc of the pinned word failed");
  }
  return RHMC_OK;
}

// The stepwise path: per step gradient -> update -> energy -> test, with the
// library's K = 1 launches; every 16 steps the count of seeds still
// descending comes back through pinned memory and ends the loop at 0.
int run_peaks_stepwise(rhmc_ctx* ctx, const Consts& c, const rhmc_peaks_opts& o, double* d_q,
                       int64_t n, int32_t* d_steps, int32_t* d_status, double* d_V,
                       hipStream_t s) {
  int rc;
  Plan gp;
  if ((rc = plan_for(ctx, c, Op::Gradient, 1, n, &gp))) return rc;
  const size_t qb = ((size_t)n * 3 * sizeof(double) + 255) & ~(size_t)255;
  const size_t eb = ((size_t)n * sizeof(double) + 255) & ~(size_t)255;
  if ((rc = ensure_mh_scratch(ctx, 2 * qb + 5 * eb + 256))) return rc;
  if ((rc = ensure_pin(ctx))) return rc;
  char* b = (char*)ctx->mh_scratch;
  PeaksStepArgs a;
  a.q = d_q;
  double* grad = (double*)b;
  a.grad = grad;
  a.q_new = (double*)(b + qb);
  double* V_new = (double*)(b + 2 * qb);
  a.V_new = V_new;
  a.V_prev = (double*)(b + 2 * qb + eb);
  a.V_last = (double*)(b + 2 * qb + 2 * eb);
  a.steps = (int32_t*)(b + 2 * qb + 3 * eb);
  a.status = (int32_t*)(b + 2 * qb + 4 * eb);
  a.n_active = (int32_t*)(b + 2 * qb + 5 * eb);
  a.n = n;
  a.f_lim = o.f_lim;
  a.dt_f_coeff = o.dt_f_coeff;
  a.dt_xy_coeff = o.dt_xy_coeff;
  a.rel_tol = o.rel_tol;
  a.n_step = o.n_step;
  a.step = 0;
  const dim3 grid((unsigned)((n + 255) / 256)), block(256);
  const int f_pos = RHMC_V_NO_POSCHECK;            // V_single has no support check
  if ((rc = launch_energy(ctx, c, d_q, nullptr, a.V_prev, nullptr, n, 1, f_pos, s))) return rc;
  hipLaunchKernelGGL(peaks_begin_kernel, grid, block, 0, s, a);
  HIP_TRY(hipGetLastError());
  for (int i = 0; i < o.n_step; ++i) {
    a.step = i;
    const bool poll = i % 16 == 15;
    if ((rc = launch_gradient(ctx, gp, c, d_q, grad, n, 1, 0, s))) return rc;
    hipLaunchKernelGGL(peaks_update_kernel<0>, grid, block, 0, s, a);
    HIP_TRY(hipGetLastError());
    if ((rc = launch_energy(ctx, c, a.q_new, nullptr, V_new, nullptr, n, 1, f_pos, s))) return rc;
    if (poll) HIP_TRY(hipMemsetAsync(a.n_active, 0, sizeof(int32_t), s));
    hipLaunchKernelGGL(peaks_update_kernel<1>, grid, block, 0, s, a);
    HIP_TRY(hipGetLastError());
    if (poll) {
      HIP_TRY(hipMemcpyAsync(ctx->h_pin, a.n_active, sizeof(int32_t), hipMemcpyDeviceToHost, s));
      HIP_TRY(hipStreamSynchronize(s));
      if (*ctx->h_pin == 0) break;
    }
  }
  hipLaunchKernelGGL(peaks_end_kernel, grid, block, 0, s, a, d_steps, d_status, d_V);
  return launch_status();
}

int launch_find_peaks(rhmc_ctx* ctx, const rhmc_params* P, const rhmc_peaks_opts* o, double* d_q,
                      int64_t n, int32_t* d_steps, int32_t* d_status, double* d_V,
                      hipStream_t s) {
  Consts c;
  int rc = make_consts(P, &c);
  if (rc) return rc;
  c.use_prior = 0;                                 // V_single / dVdq_single have neither
  c.use_Vc = 0;
  c.f_lim = o->f_lim;
  HIP_TRY(hipSetDevice(ctx->device));
  Plan pl;
  if ((rc = plan_for(ctx, c, Op::Peaks, 1, n, &pl))) return rc;
  if (pl.family != Family::RegWin1)
    return run_peaks_stepwise(ctx, c, *o, d_q, n, d_steps, d_status, d_V, s);
  const PeaksArgs k{d_q, d_steps, d_status, d_V, ctx->d_D, pl.f32 ? ctx->d_Df : nullptr, n,
                    o->f_lim, o->dt_f_coeff, o->dt_xy_coeff, o->rel_tol, o->n_step, /*pad*/ 0, c};
  return launch_k1_w28(ctx, pl, n, [&](auto img, auto dt, dim3 grid, dim3 block, size_t lds) {
    using DT = typename decltype(dt)::type;
    hipLaunchKernelGGL((peaks_k1_tiledr<decltype(img)::value, DT>), grid, block, lds, s, k);
  });
}

// ---------------------------------------------------------------------------
// HMC_find_best_dt's trials (rhmc_dt.hpp)
// ---------------------------------------------------------------------------

// The arguments both entry points share; the record's members may be NULL.
struct DtCall {
  const double* bg;
  int32_t n_bg;
  const int32_t* bg_index;
  const double *q0, *dt;
  const int32_t* flux_only;
  int64_t n;
  const double* z;
  const int32_t* steps;
  const double* lnu;
  uint64_t seed;
  const uint64_t* stream_id;
  int32_t* n_accept;
  rhmc_dt_record rec;
};

template <int LANES, int PPL>
void launch_dt_kernel(const DtArgs& a, unsigned blocks, hipStream_t s) {
  const size_t lds = PPL > 0 ? (size_t)(2 * a.side + 1) * sizeof(double2) : 0;
  hipLaunchKernelGGL((dt_trials_kernel<LANES, PPL>), dim3(blocks), dim3(LANES), lds, s, a);
}

int launch_dt_trials(rhmc_ctx* ctx, const rhmc_params* P, const rhmc_dt_opts* o, const DtCall& k,
                     hipStream_t s) {
  Consts c;
  int rc = make_consts(P, &c);
  if (rc) return rc;
  const DtPlan pl = select_dt(select_in(ctx));
  if (pl.message) return fail(RHMC_ERR_UNSUPPORTED, pl.message);
  HIP_TRY(hipSetDevice(ctx->device));
  DtArgs a;
  a.D = ctx->d_D;
  a.bg = k.bg;
  a.bg_index = k.bg_index;
  a.q0 = k.q0;
  a.dt = k.dt;
  a.flux_only = k.flux_only;
  a.z = k.z;
  a.steps = k.steps;
  a.lnu = k.lnu;
  a.stream_id = k.stream_id;
  a.n_accept = k.n_accept;
  a.r_dE = k.rec.dE;
  a.r_accept = k.rec.accept;
  a.r_q = k.rec.q;
  a.r_z = k.rec.z;
  a.r_steps = k.rec.steps;
  a.r_lnu = k.rec.lnu;
  a.gtab = nullptr;
  a.n = k.n;
  a.seed = k.seed;
  a.n_iter = o->n_iter;
  a.grad = o->grad;
  a.steps_min = o->steps_min;
  a.steps_max = o->steps_max;
  a.side = ctx->rows;
  a.n_bg = k.n_bg;
  a.inv_two_sig2 = c.inv_two_sig2;
  a.inv_norm = c.inv_norm;
  a.inv_var = c.inv_var;
  const unsigned blocks = (unsigned)std::min<int64_t>(k.n, pl.blocks_cap);
  if (pl.ppl == 0) {                               // the workgroups' factor tables
    const size_t need = (size_t)blocks * (2 * (size_t)a.side + 1) * sizeof(double2);
    if (grow(&ctx->dt_tab, &ctx->dt_tab_bytes, need) == RHMC_ERR_NOMEM)
      return fail(RHMC_ERR_NOMEM, "hipMalloc of the dt_trials factor tables failed");
    a.gtab = (double2*)ctx->dt_tab;
  }
  if (pl.lanes == 256) {
    switch (pl.ppl) {
      case 4: launch_dt_kernel<256, 4>(a, blocks, s); break;
      case 9: launch_dt_kernel<256, 9>(a, blocks, s); break;
      case 16: launch_dt_kernel<256, 16>(a, blocks, s); break;
      default: launch_dt_kernel<256, 0>(a, blocks, s); break;
    }
  } else {
    switch (pl.ppl) {
      case 16: launch_dt_kernel<64, 16>(a, blocks, s); break;
      default: launch_dt_kernel<64, 0>(a, blocks, s); break;
    }
  }
  return launch_status();
}

// Model image / Poisson realisations (rhmc_datagen.hpp) into d_out
// [max(n_real,1)][rows][cols].
int launch_gen_image(rhmc_ctx* ctx, const rhmc_params* P, const double* d_q, int32_t K,
                     int32_t rows, int32_t cols, int32_t n_real, uint64_t seed, double* d_out,
                     hipStream_t s) {
  DataArgs a;
  int rc = make_consts(P, &a.c);
  if (rc) return rc;
  if (K < 0 || K > (1 << 20)) return fail(RHMC_ERR_ARG, "K must be in [0, 2^20]");
  if (rows < 1 || cols < 1) return fail(RHMC_ERR_ARG, "rows/cols must be >= 1");
  if (n_real < 0) return fail(RHMC_ERR_ARG, "n_real < 0");
  if (K > 0 && !d_q) return fail(RHMC_ERR_ARG, "q is NULL");
  if (!d_out) return fail(RHMC_ERR_ARG, "out is NULL");
  const int64_t npix = (int64_t)rows * cols;
  const int64_t total = npix * (n_real > 0 ? n_real : 1);
  if (total > ((int64_t)1 << 36)) return fail(RHMC_ERR_ARG, "rows*cols*n_real too large");
  a.q = d_q;
  a.out = d_out;
  a.K = K;
  a.rows = rows;
  a.cols = cols;
  a.poisson = n_real > 0;
  a.n_real = n_real;
  a.seed = seed;
  HIP_TRY(hipSetDevice(ctx->device));
  const dim3 grid((unsigned)((total + 255) / 256)), block(256);
  hipLaunchKernelGGL(datagen_kernel, grid, block, 0, s, a);
  return launch_status();
}

}  // namespace
