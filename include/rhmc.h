/*
 * rhmc.h — C-ABI of the MI355X-native RHMC leapfrog engine (librhmc.so).
 *
 * Drop-in boundary for ONE hot path of jaekor91/HMC-stellar-toy-model: the
 * implicit generalized-leapfrog step of the Riemannian-HMC sampler for the
 * Poisson / Gaussian-PSF stellar-photometry posterior.
 *
 * Reference interface each entry point replaces (file:line into the
 * reference checkout):
 *   rhmc_leapfrog / rhmc_leapfrog_device
 *       base_class.RHMC_single_step(q, p, delta, counter_max)
 *       sampler_RHMC.py:522-566, called Nsteps times per MH iteration from
 *       multi_gym.run_RHMC (sampler_RHMC.py:1053-1054) and inlined in
 *       single_gym.run_single_RHMC solver="implicit" (:729-772).
 *       n_steps consecutive steps are fused into one launch.
 *   rhmc_gradient
 *       base_class.dVdq (sampler_RHMC.py:365-425) and base_class.dphidq
 *       (:448-465), batched over chains.
 *   rhmc_energy / rhmc_energy_device
 *       base_class.V (sampler_RHMC.py:294-351) and base_class.T (:353-363)
 *       at H(q) (:229-258) — the trajectory-endpoint energies of the MH test
 *       (:1021-1026, :1070-1071).
 *   rhmc_mh / rhmc_mh_device
 *       multi_gym.run_RHMC, move-0 ("within") branch (sampler_RHMC.py:1018-1083):
 *       momentum draw p = z*sqrt(H(q)) (:1021-1022), E0 = V + T (:1025-1027),
 *       Nsteps leapfrog steps (:1053-1054), E1, accept if dE < 0 or
 *       ln u < -dE (:1072-1083) — n_iter iterations, all on the device.
 *       rhmc_mh_scheduled(_device): the same with run_RHMC's schedule_g_ff2 /
 *       schedule_beta (:1010-1016).
 *   rhmc_integrate / rhmc_integrate_device
 *       the reference's other integrators, selected by RHMC_SOLVER_*:
 *       single_gym.run_single_HMC leapfrog (sampler_RHMC.py:628-645) and
 *       single_gym.run_single_RHMC solver="naive" (:690-708) / "leap_frog"
 *       (:709-728); RHMC_SOLVER_IMPLICIT is RHMC_single_step.
 *   rhmc_ctx_create / rhmc_ctx_set_image
 *       the instance attribute base_class.D set by gen_mock_data
 *       (sampler_RHMC.py:77-99); uploaded once per context.
 *   rhmc_gen_image / rhmc_gen_image_device
 *       base_class.gen_model (sampler_RHMC.py:101-116), gen_mock_data
 *       (:77-99, Poisson draw utils.py:488-496) and the N_trial realisations
 *       of gen_noise_profile (:118-144), on the device.
 *   rhmc_leapfrog_ragged_device / rhmc_energy_ragged_device /
 *   rhmc_rows_copy_device / rhmc_kinetic_rows_device (ABI 4)
 *       the same step and V for chains of DIFFERENT star counts in one launch,
 *       and the momentum draw / T of run_RHMC (:1021-1026, :353-363) on
 *       device-resident ragged sets: the reversible-jump iterations of
 *       run_RHMC (:1018-1187), whose chains change K by births, deaths,
 *       splits and merges (librhmc_rj.so keeps them in HBM between phases).
 *   rhmc_find_peaks / rhmc_find_peaks_device
 *       samplers.lightsource_gym.find_peaks' gradient descent of the grid
 *       seeds (samplers.py:190-221) on V_single / dVdq_single (:77-127)
 *       against the pure-background model; the seed grid (:157-180) and the
 *       merge of near-duplicates (:232-252) stay on the host.
 *   rhmc_dt_trials / rhmc_dt_trials_device
 *       the trial of samplers.lightsource_gym.HMC_find_best_dt's step-size
 *       search (samplers.py:332-371): Metropolis iterations of explicit
 *       leapfrog on one star against a background image; the coarse / fine
 *       search around the trials (:327-456) stays on the host.
 *   rhmc_diag_random / rhmc_diag_random_device
 *       the trajectory of samplers.lightsource_gym.RHMC_random_diag
 *       (samplers.py:766-800): explicit leapfrog under the flux-dependent
 *       diagonal mass matrix of mass_matrix / F / G / dlnDetdq / dpMpdq
 *       (:574-664); the momentum draw, E, K and the MH test (:719-823) stay on
 *       the host.
 *   rhmc_hess_derivs / rhmc_hess_random (and their _device forms)
 *       samplers.lightsource_gym.RHMC_random (samplers.py:930-1105): the
 *       derivative sets dVdq, dVdqq, dVdqqq and V of
 *       RHMC_efficient_computation (:828-927) and the trajectory under the
 *       Hessian-diagonal metric (:1016-1067); the momentum draw, E and the MH
 *       test stay on the host.
 *   rhmc_params
 *       the instance attributes the step reads: dt, g_xx,
 *       g_ff, g_ff2, g0, g1, g2, B_count, f_lim, mB (-> f_low),
 *       PSF_FWHM_pix, use_prior, alpha, use_Vc, beta, Vc_r_pow, plus the
 *       run_RHMC arguments delta / counter_max (:937-939).
 *
 * Conventions
 *   - Arrays are C-contiguous fp64 [n_chains][3K] with (f_k, x_k, y_k)
 *     interleaved per star, flux in counts (format_q, sampler_RHMC.py:209).
 *     D is fp64 [rows][cols], rows == cols (reference limitation:
 *     gauss_PSF returns (cols, rows), utils.py:481-483).
 *   - Host-pointer entry points are synchronous and update q, p in place.
 *     The *_device entry points take device pointers and a hipStream_t
 *     (passed as void*, NULL = the context's stream) and are asynchronous.
 *   - Every call returns 0 on success or a negative RHMC_ERR_* code;
 *     rhmc_last_error() gives a thread-local message.  No C++ exception
 *     crosses the ABI.  A context must not be used by two threads at once,
 *     except that rhmc_leapfrog_device, rhmc_energy_device,
 *     rhmc_leapfrog_ragged_device, rhmc_energy_ragged_device,
 *     rhmc_rows_copy_device, rhmc_kinetic_rows_device and rhmc_ragged_ok
 *     (which read the context's options and image and otherwise touch only a
 *     per-stream, mutex-guarded table buffer) may be called from several
 *     threads at once, on the same or distinct streams: a launch holds a
 *     reference to the table buffer it was given until it is enqueued, so a
 *     buffer grown by another thread is released only after that launch (the
 *     order of two threads' launches on one stream is theirs to arrange).
 *     Options must not change while such calls run.  One context per GPU.
 *     rhmc_diag_random and rhmc_diag_random_device are NOT among them (like
 *     rhmc_hmc_random, whose plan and launch shapes they share): one thread
 *     per context; the host-pointer call stages through the context's scratch
 *     buffer and returns after its stream has drained, the device-pointer
 *     call only enqueues on `stream` and reads opts before it returns.
 */
#ifndef RHMC_H
#define RHMC_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define RHMC_ABI_VERSION 4

enum {
  RHMC_OK = 0,
  RHMC_ERR_ARG = -1,         /* bad argument (shape, NULL, K range ...) */
  RHMC_ERR_HIP = -2,         /* a HIP runtime call failed                */
  RHMC_ERR_NOMEM = -3,       /* device allocation failed                 */
  RHMC_ERR_UNSUPPORTED = -4  /* configuration not built into this library */
};

/* Integrators selectable through rhmc_integrate. */
enum {
  RHMC_SOLVER_IMPLICIT = 0,       /* RHMC_single_step (:522-566)                  */
  RHMC_SOLVER_HMC = 1,            /* plain leapfrog, unit metric (:628-645)       */
  RHMC_SOLVER_RHMC_NAIVE = 2,     /* explicit RHMC, "naive" (:690-708)            */
  RHMC_SOLVER_RHMC_LEAPFROG = 3   /* explicit RHMC, "leap_frog" (:709-728)        */
};

/* Per-chain status bits written by rhmc_leapfrog (OR over all steps). */
#define RHMC_STATUS_NONFINITE   1u  /* q or p became NaN/inf                    */
#define RHMC_STATUS_PLOOP_CAP   2u  /* p fixed-point loop stopped at counter_max */
#define RHMC_STATUS_QLOOP_CAP   4u  /* q fixed-point loop stopped at counter_max */
#define RHMC_STATUS_REFLECT_F   8u  /* flux-wall reflection (:558-559)           */
#define RHMC_STATUS_REFLECT_XY 16u  /* edge reflection (:561-564)                */
/* A reflection of the implicit step fired with its coordinate within 2^-40 (9.1e-13) of
 * the wall (relative to max(1, |wall|): f_lim, 0 or R-1; :554-564).  Such a
 * chain can legitimately reflect the other way on a last-bit difference
 * (SURVEY §8(c)), so callers report these chains separately. */
#define RHMC_STATUS_NEAR_WALL  32u
/* How a seed of rhmc_find_peaks stopped: exactly one of the three per seed,
 * in bits the step's status bits above do not use (RHMC_STATUS_NONFINITE may
 * come with them). */
#define RHMC_PEAK_CONVERGED  256u  /* |(V - V_prev)/V_prev| < rel_tol (samplers.py:215) */
#define RHMC_PEAK_FAINT      512u  /* f < f_lim after an update (:209-211)              */
#define RHMC_PEAK_CAP       1024u  /* n_step steps without either                       */

/* Instance state read by the step (POD; all fp64 except the flags). */
typedef struct rhmc_params {
  double dt;           /* self.dt                                            */
  double delta;        /* fixed-point tolerance (absolute, max-norm)         */
  double B_count;      /* background counts per pixel                        */
  double f_lim;        /* flux wall (counts)                                 */
  double f_low;        /* H_xx clamp = mag2flux(mB+2)*flux_to_count (:267)   */
  double fwhm_pix;     /* PSF FWHM in pixels                                 */
  double g_xx, g_ff, g_ff2;
  double g0, g1, g2;   /* metric factors (utils.factors at 48x48, :165)      */
  double alpha;        /* prior exponent (used when use_prior)               */
  double beta;         /* repulsion strength (used when use_Vc)              */
  double Vc_r_pow;     /* repulsion power                                    */
  double V_prior_const;/* rhmc_energy only: the cached prior constant (:321) */
  int32_t counter_max; /* fixed-point iteration cap                          */
  int32_t use_prior;
  int32_t use_Vc;
  int32_t reserved;    /* must be 0                                          */
} rhmc_params;

typedef struct rhmc_ctx rhmc_ctx;

/*
 * Context options (rhmc_ctx_set_option).  Nothing in the library reads the
 * environment: kernel selection is per context, AUTO unless a caller (the
 * parity tests) sets it.
 *
 * RHMC_OPT_KERNEL: the kernel family the compute calls use.  A family that
 * does not serve the call's configuration (K, image side, PSF width, fp32
 * exactness of the image) leaves the automatic choice for that call.
 *   AUTO            the default dispatch
 *   GENERIC         one wave per chain, image in LDS (K <= 16, image + tables
 *                   fit LDS; else WINDOWED); explicit integrators and
 *                   HMC_random take WINDOWED; MH runs the four-kernel loop
 *   WINDOWED        one wave per chain, 32-px star windows, image in HBM/L2
 *   REGWIN          K = 1 register-window kernel at every batch size
 *   REGWIN32        ... forced onto the 32-px window
 *   REGWIN_F64      ... with an fp64 pixel cache
 *   LANE1 / LANE4   K = 1 lane-group kernel, 1 / 4 lanes per chain, at every
 *                   batch size; LANE1_F64: fp64 image in LDS
 *   PIXMAJOR        2 <= K <= 10 pixel-major kernel (the AUTO choice there)
 *   MULTIWIN        K >= 2 multi-star register-window kernel (also where the
 *                   pixel-major kernel would serve); MULTIWIN_NOTAB without
 *                   the LDS factor tables
 *   DENSE           the many-star kernel for 32/48-px images (full-image
 *                   pixel-major Lambda, star-major sums; the AUTO choice there
 *                   from 11 stars) at any K
 * RHMC_OPT_MH_FUSED: 1 (default) = one-launch MH where a fused kernel exists,
 *   0 = the four-kernel loop (begin / leapfrog / energy / end) always.
 * RHMC_OPT_WINDOW_SPLIT: waves per chain pair in the multi-star
 *   register-window kernel's implicit step (leapfrog_kr): 0 (default) = by
 *   batch size (1 from 8 waves per SIMD up, else 2 or 4, so that e.g. C5's
 *   8192 chains split over 8 GPUs still fill each one), or 1, 2, 4.  The
 *   results do not depend on it (bit-identical).  It applies only where that
 *   kernel runs the implicit step without LDS factor tables (images larger
 *   than 64 px, or K > 16); the factor-table variant, the explicit solvers,
 *   HMC_random and every other kernel family ignore it, and
 *   rhmc_ctx_get_option returns the value set either way.
 * RHMC_OPT_TABLES (diagnostic; results do not depend on it): the windowed
 *   kernels from 65 stars keep their per-chain PSF factor tables in global
 *   memory, one buffer per (context, stream).  STREAM (default) = that
 *   buffer; STREAM_POISON = the same, filled with 0xFF bytes (NaN) before
 *   every launch, so that a read of an entry the launch did not write would
 *   show as a NaN result (tests/test_gpu_tables_determinism.py: none does).
 *   Any other value is refused with RHMC_ERR_ARG.
 * RHMC_OPT_PEAKS_FUSED: 1 (default) = rhmc_find_peaks runs the one-launch
 *   descent kernel where it exists (32/48/64-px images, a PSF narrow enough
 *   for the 28-px window, no forced per-wave family), 0 = always the stepwise
 *   path (gradient / update / energy / update launches per step).
 * RHMC_OPT_DT_LANES: lanes per task of rhmc_dt_trials, 0 (default) = the
 *   library's choice (256), 64 or 256 (the A/B of DESIGN.md section 4e).
 */
enum {
  RHMC_OPT_KERNEL = 1,
  RHMC_OPT_MH_FUSED = 2,
  RHMC_OPT_WINDOW_SPLIT = 3,
  RHMC_OPT_TABLES = 4,
  RHMC_OPT_PEAKS_FUSED = 5,
  RHMC_OPT_DT_LANES = 6
};
enum {
  RHMC_TABLES_STREAM = 0,
  RHMC_TABLES_STREAM_POISON = 1
};
enum {
  RHMC_KERNEL_AUTO = 0,
  RHMC_KERNEL_GENERIC = 1,
  RHMC_KERNEL_WINDOWED = 2,
  RHMC_KERNEL_REGWIN = 3,
  RHMC_KERNEL_REGWIN32 = 4,
  RHMC_KERNEL_REGWIN_F64 = 5,
  RHMC_KERNEL_LANE1 = 6,
  RHMC_KERNEL_LANE4 = 7,
  RHMC_KERNEL_LANE1_F64 = 8,
  RHMC_KERNEL_PIXMAJOR = 9,
  RHMC_KERNEL_MULTIWIN = 10,
  RHMC_KERNEL_MULTIWIN_NOTAB = 11,
  RHMC_KERNEL_DENSE = 12
};
int rhmc_ctx_set_option(rhmc_ctx* ctx, int32_t option, int32_t value);
int rhmc_ctx_get_option(rhmc_ctx* ctx, int32_t option, int32_t* value);

/* ABI version of the loaded library (== RHMC_ABI_VERSION when in sync). */
int rhmc_abi_version(void);
/* Number of visible GPUs; 0 (and RHMC_OK) when none. */
int rhmc_device_count(int* n);
/* Thread-local message of the last failing call ("" if none). */
const char* rhmc_last_error(void);

/* Create a context on `device` and upload D [rows][cols] (host pointer). */
int rhmc_ctx_create(int device, const double* D, int32_t rows, int32_t cols,
                    rhmc_ctx** out);
/* Replace the data image (host pointer); may change the size. */
int rhmc_ctx_set_image(rhmc_ctx* ctx, const double* D, int32_t rows, int32_t cols);
/* Device pointer of the context's image (for callers that keep state on device). */
int rhmc_ctx_image_device(rhmc_ctx* ctx, const double** d_image);
void rhmc_ctx_destroy(rhmc_ctx* ctx);
/* Wait for all work queued on the context's stream. */
int rhmc_ctx_synchronize(rhmc_ctx* ctx);

/*
 * n_steps RHMC_single_step()s on every chain.  q, p: host [n_chains][3K],
 * updated in place.  fp_iters (nullable): host int32 [n_chains][2], the
 * p- and q-loop iteration counts summed over the n_steps steps.  status
 * (nullable): host int32 [n_chains], RHMC_STATUS_* bits.  1 <= K <= 1024 on
 * every step, gradient, energy and MH entry point (else RHMC_ERR_ARG).  From
 * 65 stars the windowed one-wave-per-chain kernels (images other than the
 * dense kernel's 32/48 px, or K > 256) keep their PSF factor tables in global
 * memory, 2 x 33 doubles per star per chain in a buffer the context keeps
 * per stream until rhmc_ctx_destroy (grown on demand after a sync of that
 * stream; RHMC_ERR_NOMEM if that fails); they need a PSF narrow
 * enough for the 32-pixel window (else RHMC_ERR_UNSUPPORTED).
 */
int rhmc_leapfrog(rhmc_ctx* ctx, const rhmc_params* P, double* q, double* p,
                  int64_t n_chains, int32_t K, int32_t n_steps,
                  int32_t* fp_iters, int32_t* status);

/* Same on device-resident buffers, asynchronous on `stream` (hipStream_t). */
int rhmc_leapfrog_device(rhmc_ctx* ctx, const rhmc_params* P, double* d_q,
                         double* d_p, int64_t n_chains, int32_t K,
                         int32_t n_steps, int32_t* d_fp_iters,
                         int32_t* d_status, void* stream);

/*
 * Ragged chain sets (ABI 4).  Chain i of a call is row rows[i] (d_rows NULL:
 * row i) of padded device arrays [*][ld]; the row holds the chain's d_K[row]
 * stars (its first 3 K entries; d_K indexed by row).  One launch serves every
 * star count in [K_min, K_max] when the automatic dispatch runs a slotted
 * one-wave-per-chain kernel for each of them — the dense kernel on 32/48-px
 * images from 11 stars, the windowed kernel — or the pixel-major kernel (2-10
 * stars on 32/48-px images whose pixels are exact in fp32; a launch takes one
 * family: 2-10 and 11+ stars are separate sets) (rhmc_ragged_ok says which K);
 * K_min and K_max must need the same register slots (1-64, 65-128, 129-256,
 * 257-512, 513-1024 stars), else RHMC_ERR_ARG, and a K the slotted kernels do not serve gives
 * RHMC_ERR_UNSUPPORTED.  Each chain's results equal those of a fixed-K call
 * on it (the kernels are batch-invariant).  Entries of a row past 3 d_K[row],
 * rows not in d_rows, and d_K of such rows are neither read nor written
 * (tests/test_gpu_ragged_bodies.py pins this for every kernel body of the
 * step, tests/test_gpu_energy_bodies.py for the energy).  Asynchronous on
 * `stream`.
 */
int rhmc_ragged_ok(rhmc_ctx* ctx, const rhmc_params* P, int32_t K, int32_t* ok);
/* n_steps RHMC_single_step()s on the set; q, p rows updated in place. */
int rhmc_leapfrog_ragged_device(rhmc_ctx* ctx, const rhmc_params* P, double* d_q, double* d_p,
                                int64_t ld, const int64_t* d_rows, const int32_t* d_K,
                                int64_t n, int32_t K_min, int32_t K_max, int32_t n_steps,
                                void* stream);
/* V (rhmc_energy's, f_pos bits likewise) of the set: d_V[i] for chain i. */
int rhmc_energy_ragged_device(rhmc_ctx* ctx, const rhmc_params* P, const double* d_q, int64_t ld,
                              const int64_t* d_rows, const int32_t* d_K, int64_t n,
                              int32_t K_min, int32_t K_max, int32_t f_pos, double* d_V,
                              void* stream);
/* dst[dst_rows[i]][0:width] = src[src_rows[i]][0:width] for i < n (either
 * index array NULL: row i): gathers of a ragged set into packed [n][3K]
 * batches for the fixed-K entry points, scatters back, row restores. */
int rhmc_rows_copy_device(rhmc_ctx* ctx, const double* d_src, int64_t ld_src,
                          const int64_t* d_src_rows, double* d_dst, int64_t ld_dst,
                          const int64_t* d_dst_rows, int64_t n, int32_t width, void* stream);
/* Rows 0..n-1 of a ragged set (d_K[c] stars): with d_z non-NULL first the
 * momentum draw p = z sqrt(H(q)) (:1021-1022; chain c's 3 K normals at
 * d_z + d_zoff[c], p zeroed past 3 K), then T[c] = (sum p^2/H(q) + sum
 * ln|H(q)|) / 2 (:353-363) with NumPy's pairwise summation order.  H
 * follows the reference's operation order (:260-292, g_ff2 / g_xx / B /
 * f_low from P).  1 <= d_K[c] <= 1024 (a larger count gets T = NaN). */
int rhmc_kinetic_rows_device(rhmc_ctx* ctx, const rhmc_params* P, const double* d_q, double* d_p,
                             int64_t ld, const int32_t* d_K, const double* d_z,
                             const int64_t* d_zoff, int64_t n, double* d_T, void* stream);

/* kind: 0 = dVdq (:365-425), 1 = dphidq (:448-465).  Host pointers. */
int rhmc_gradient(rhmc_ctx* ctx, const rhmc_params* P, const double* q,
                  double* grad, int64_t n_chains, int32_t K, int32_t kind);

/* V (:294-351) and T at H(q) (:353-363) per chain.  V or T may be NULL.  p
 * may be NULL when T is NULL.  Host pointers.  f_pos is a bit set:
 * RHMC_V_FLUX_WALL (1) = V is inf when a flux is below f_lim (:303-309, the
 * reference's f_pos=True); RHMC_V_NO_POSCHECK (2) = skip the position support
 * check (:311-317), i.e. samplers.lightsource_gym.V (samplers.py:1137-1150),
 * which has none. */
#define RHMC_V_FLUX_WALL   1
#define RHMC_V_NO_POSCHECK 2
int rhmc_energy(rhmc_ctx* ctx, const rhmc_params* P, const double* q,
                const double* p, double* V, double* T, int64_t n_chains,
                int32_t K, int32_t f_pos);
/* Same on device-resident buffers (d_V or d_T may be NULL; d_p may be NULL
 * when d_T is), asynchronous on `stream` (hipStream_t; NULL = the context's
 * stream).  Launches on distinct streams may run concurrently. */
int rhmc_energy_device(rhmc_ctx* ctx, const rhmc_params* P, const double* d_q,
                       const double* d_p, double* d_V, double* d_T, int64_t n_chains,
                       int32_t K, int32_t f_pos, void* stream);

/* n_steps steps of integrator `solver` (RHMC_SOLVER_*) on every chain; q, p
 * host [n_chains][3K], updated in place.  f_pos: the flux-wall momentum flip of
 * the explicit RHMC solvers (:698-705, :719-726).  status nullable. */
int rhmc_integrate(rhmc_ctx* ctx, const rhmc_params* P, int32_t solver, double* q, double* p,
                   int64_t n_chains, int32_t K, int32_t n_steps, int32_t f_pos,
                   int32_t* status);
int rhmc_integrate_device(rhmc_ctx* ctx, const rhmc_params* P, int32_t solver, double* d_q,
                          double* d_p, int64_t n_chains, int32_t K, int32_t n_steps,
                          int32_t f_pos, int32_t* d_status, void* stream);

/* samplers.lightsource_gym.HMC_random's trajectory (samplers.py:519-552;
 * the MH bookkeeping around it, :489-568, stays on the host): unit-mass
 * leapfrog with the per-coordinate step vector dt[3K] (the reference's
 * self.dt) and steps[c] >= 1 steps for chain c (its np.random.randint draw),
 * flux wall at P->f_lim with the reference's quirks (sticky flip mask; when
 * the last step flipped, p is left at its input value and the chain's status
 * gets RHMC_STATUS_REFLECT_F).  q, p host [n_chains][3K] updated in place;
 * status nullable.  Gradient: dVdq without metric (:1108-1135). */
int rhmc_hmc_random(rhmc_ctx* ctx, const rhmc_params* P, const double* dt, double* q, double* p,
                    const int32_t* steps, int64_t n_chains, int32_t K, int32_t* status);
int rhmc_hmc_random_device(rhmc_ctx* ctx, const rhmc_params* P, const double* d_dt,
                           double* d_q, double* d_p, const int32_t* d_steps, int64_t n_chains,
                           int32_t K, int32_t* d_status, void* stream);

/* samplers.lightsource_gym.RHMC_random_diag's trajectory (samplers.py:766-800;
 * the MH bookkeeping around it, :719-823, stays on the host): explicit leapfrog
 * under the flux-dependent diagonal mass matrix M = diag(1/f, f factor1,
 * f factor1) per star (mass_matrix / F / G, :574-634) with the one step
 * opts->dt (the reference's dt_global) and steps[c] >= 1 steps for chain c:
 *   p_half = p - dt/2 F(q, p),   F = dVdq + dlnDetdq + dpMpdq (:636-664)
 *   per step: q += dt p_half / M(q before the update); p_half -= dt F(q, p)
 *   at the end: p = p_half + dt/2 F(q, p)
 * with the reference's quirks: dpMpdq takes the momentum the call STARTED
 * with on every step (never p_half); the flux wall at P->f_lim behaves as in
 * rhmc_hmc_random (sticky flip mask; when the last step flipped, p is left at
 * its input value and the chain's status gets RHMC_STATUS_REFLECT_F); a NaN
 * flux does not flip.  RHMC_STATUS_NONFINITE marks a non-finite result.
 * factor1 is utils.factors()'s second value (compute_factors, :69-75).
 * trace (nullable) [n_chains][opts->trace_rows][3K]: row t receives q after
 * step t (row 0: the start) for t <= steps[c]; later rows are left untouched.
 * trace_rows must exceed the longest trajectory (checked by the host-pointer
 * call; the device-pointer call cannot read steps and writes no row past
 * trace_rows).  q, p [n_chains][3K] updated in place; status nullable.  Only
 * B_count, f_lim, the PSF width and the prior switch of P are read. */
typedef struct rhmc_diag_opts {
  double dt;          /* dt_global (finite)                            */
  double factor1;     /* F(f) = f factor1 (finite, > 0)                */
  int32_t trace_rows; /* rows per chain of `trace` (ignored without it) */
  int32_t reserved;   /* must be 0                                     */
} rhmc_diag_opts;
int rhmc_diag_random(rhmc_ctx* ctx, const rhmc_params* P, const rhmc_diag_opts* opts, double* q,
                     double* p, const int32_t* steps, int64_t n_chains, int32_t K,
                     int32_t* status, double* trace);
int rhmc_diag_random_device(rhmc_ctx* ctx, const rhmc_params* P, const rhmc_diag_opts* opts,
                            double* d_q, double* d_p, const int32_t* d_steps, int64_t n_chains,
                            int32_t K, int32_t* d_status, double* d_trace, void* stream);

/* samplers.lightsource_gym.RHMC_random (samplers.py:930-1105): the sampler
 * whose mass matrix is the diagonal of the likelihood's Hessian, dVdqq, with
 * the third derivatives dVdqqq in its force.  Two operations, both of one
 * kernel family (csrc/rhmc_hess.hpp: one wave per chain over the full image),
 * which serves 1 <= K <= 16 on square images of side 16..48 and returns
 * RHMC_ERR_UNSUPPORTED for everything else; RHMC_OPT_KERNEL does not affect it.
 * Only B_count, f_lim and the PSF width of P are read (no prior, no metric
 * constants).
 *
 * rhmc_hess_derivs: RHMC_efficient_computation's three derivative sets
 * (:840-903) at q [n_chains][3K], per star (f, x, y):
 *   dVdq   = (S r1 P,       f S r1 Px,                  ...y)
 *   dVdqq  = (S r2 P^2,     f^2 S r2 Px^2 + f S r1 Pxx, ...y)
 *   dVdqqq = (-2 S r3 P^3, -f^3 S r3 Px^3 + 3 f^2 S r2 Px Pxx + f S r1 Pxxx, ...y)
 * with r0 = D / Lambda, r1 = 1 - r0, r2 = r0 / Lambda, r3 = r2 / Lambda and S
 * the sum over the whole image, and V = -S (D ln Lambda - Lambda) [n_chains].
 * There is no wall check (the reference's dVdqq_only form).  dVdq, dVdqq,
 * dVdqqq and V are each nullable.
 *
 * rhmc_hess_random: the trajectory (:1016-1067) of steps[c] >= 1 steps from
 * (q, p), with dt = (dt_f, dt_xy, dt_xy) per star:
 *   at a derivative set: dqdt = p / dVdqq,
 *                        dpdt = -dVdqqq (1 / dVdqq - dqdt^2) / 2 - dVdq,
 *                        or +inf for every coordinate when some f < f_lim
 *   p_half = p + dt dpdt(q, p) / 2
 *   per step: stop if E(q, p_half) == +inf; q += dt dqdt(q, p_half);
 *             p_half += dt' dpdt(new q, p_half), dt' = dt / 2 on the last step
 * and the reference's quirks (csrc/rhmc_traj.hpp lists them): dVdqq is used
 * as it comes, negative or zero included; the position flags are set for every
 * coordinate below the image side, so px and py of a star inside the image
 * are replaced by their negatives on every step; flags are sticky per star
 * and applied when any star of the chain sets one in that step; after a wall
 * crossing the unflagged momenta become +-inf (NaN with a zero step) and the
 * next step stops; there is no closing half step.  The stop test needs no
 * logarithm per pixel because V is never +-inf while f_lim >= 0: E == +inf
 * iff some f < f_lim, or K = S p^2 / dVdqq / 2 + ln(prod dVdqq) / 2 is +inf
 * and every coordinate of q is finite.  THEREFORE P->f_lim < 0 IS REFUSED
 * (RHMC_ERR_ARG) by both rhmc_hess_random entry points.
 * q and p are updated in place: q is the end state, p is p_half as the
 * reference leaves it.  steps_done[c] (nullable) is the number of completed
 * steps, below steps[c] iff the trajectory stopped early.  status (nullable):
 * RHMC_STATUS_REFLECT_F when a flux flag was set, RHMC_STATUS_REFLECT_XY when
 * a position flag was set, RHMC_STATUS_NONFINITE for a non-finite q or p.
 * dVdq, dVdqq, dVdqqq (each nullable) receive the derivative sets AT THE END
 * STATE, bit for bit what rhmc_hess_derivs gives there.
 * RHMC_ERR_ARG: NULL ctx, P, opts, steps, or q / p with n_chains > 0; a
 * non-finite step; reserved != 0; f_lim < 0; K outside 1..1024; steps[c] < 1
 * (host-pointer call only; the device-pointer call cannot read steps, and a
 * chain with steps < 1 there gets the first half kick alone).  n_chains = 0
 * is a no-op.  One thread per context, like rhmc_diag_random. */
typedef struct rhmc_hess_opts {
  double dt_f;         /* dt_RHMC_f (finite)  */
  double dt_xy;        /* dt_RHMC_xy (finite) */
  int32_t reserved[2]; /* must be 0           */
} rhmc_hess_opts;
int rhmc_hess_derivs(rhmc_ctx* ctx, const rhmc_params* P, const double* q, double* dVdq,
                     double* dVdqq, double* dVdqqq, double* V, int64_t n_chains, int32_t K);
int rhmc_hess_derivs_device(rhmc_ctx* ctx, const rhmc_params* P, const double* d_q,
                            double* d_dVdq, double* d_dVdqq, double* d_dVdqqq, double* d_V,
                            int64_t n_chains, int32_t K, void* stream);
int rhmc_hess_random(rhmc_ctx* ctx, const rhmc_params* P, const rhmc_hess_opts* opts, double* q,
                     double* p, const int32_t* steps, int64_t n_chains, int32_t K,
                     int32_t* status, int32_t* steps_done, double* dVdq, double* dVdqq,
                     double* dVdqqq);
int rhmc_hess_random_device(rhmc_ctx* ctx, const rhmc_params* P, const rhmc_hess_opts* opts,
                            double* d_q, double* d_p, const int32_t* d_steps, int64_t n_chains,
                            int32_t K, int32_t* d_status, int32_t* d_steps_done, double* d_dVdq,
                            double* d_dVdqq, double* d_dVdqqq, void* stream);

/* Per-iteration records of rhmc_mh (all nullable; host pointers for rhmc_mh,
 * device pointers for rhmc_mh_device).  Row l holds the state at the START
 * of iteration l, like the reference's q_chain / E_chain / V_chain / T_chain
 * (:1038-1042); accept[l] is A_chain[l] (:1077). */
typedef struct rhmc_mh_record {
  double* q_chain;   /* [n_iter][n_chains][3K] */
  double* E_chain;   /* [n_iter][n_chains] */
  double* V_chain;   /* [n_iter][n_chains] */
  double* T_chain;   /* [n_iter][n_chains] */
  int32_t* accept;   /* [n_iter][n_chains] */
} rhmc_mh_record;

/*
 * n_iter MH iterations of n_steps leapfrog steps each on every chain; q
 * [n_chains][3K] is updated in place to the last accepted state.  Randoms:
 * z [n_iter][n_chains][3K] standard normals and u [n_iter][n_chains] uniforms
 * in (0,1] — pass the reference's own NumPy draws for bit-level parity of the
 * accept sequence; NULL draws them on the device (Philox-4x32-10, `seed`,
 * counter = (index, iteration, chain)).  P->V_prior_const must be set when
 * use_prior.
 */
int rhmc_mh(rhmc_ctx* ctx, const rhmc_params* P, double* q, int64_t n_chains, int32_t K,
            int32_t n_iter, int32_t n_steps, int32_t f_pos, const double* z, const double* u,
            uint64_t seed, const rhmc_mh_record* rec);
int rhmc_mh_device(rhmc_ctx* ctx, const rhmc_params* P, double* d_q, int64_t n_chains,
                   int32_t K, int32_t n_iter, int32_t n_steps, int32_t f_pos, const double* d_z,
                   const double* d_u, uint64_t seed, const rhmc_mh_record* rec, void* stream);

/*
 * Parameter schedules of multi_gym.run_RHMC (schedule_g_ff2 / schedule_beta,
 * sampler_RHMC.py:937-939, :1010-1016; RHMC-big-sim3.py:11-12): MH iteration
 * l of the call runs with g_ff2 = g_ff2[l] and beta = beta[l] while l < the
 * array's size, and with its last value after it; a NULL array (size 0)
 * keeps P's value.  Host arrays, for the device entry point too (they set
 * each iteration's constants).  P->g_ff2 / P->beta are not modified.
 */
typedef struct rhmc_mh_schedule {
  const double* g_ff2;  /* [n_g_ff2] or NULL */
  const double* beta;   /* [n_beta] or NULL  */
  int32_t n_g_ff2;
  int32_t n_beta;
} rhmc_mh_schedule;
/* rhmc_mh / rhmc_mh_device with a schedule (sched NULL: identical to them). */
int rhmc_mh_scheduled(rhmc_ctx* ctx, const rhmc_params* P, double* q, int64_t n_chains,
                      int32_t K, int32_t n_iter, int32_t n_steps, int32_t f_pos, const double* z,
                      const double* u, uint64_t seed, const rhmc_mh_record* rec,
                      const rhmc_mh_schedule* sched);
int rhmc_mh_scheduled_device(rhmc_ctx* ctx, const rhmc_params* P, double* d_q,
                             int64_t n_chains, int32_t K, int32_t n_iter, int32_t n_steps,
                             int32_t f_pos, const double* d_z, const double* d_u, uint64_t seed,
                             const rhmc_mh_record* rec, const rhmc_mh_schedule* sched,
                             void* stream);

/*
 * Data generation.  q: [K][3] (flux in counts, x, y), K >= 0.  n_real == 0:
 * the model image B_count + sum_k f_k PSF_k (gen_model, sampler_RHMC.py:101-116;
 * per pixel exp(-((i+.5-x)^2 + (j+.5-y)^2) / (2 sigma^2)) / (2 pi sigma^2),
 * utils.py:475-486) into out [rows][cols].  n_real >= 1: n_real independent
 * Poisson realisations of it (gen_mock_data :77-99 / gen_noise_profile
 * :130-133) into out [n_real][rows][cols]; the Poisson sampler is NumPy's
 * legacy algorithm (multiplication below lam 10, PTRS above) on Philox-4x32-10
 * keyed by `seed` and the pixel index — the same distribution as the
 * reference, not the same stream.  Only P->B_count and P->fwhm_pix are read
 * (P->reserved must be 0).  install != 0 makes image 0 the context's data
 * image without a host round trip (rows == cols); out may then be NULL.
 * rhmc_ctx_create accepts D == NULL for a context that gets its image here.
 */
int rhmc_gen_image(rhmc_ctx* ctx, const rhmc_params* P, const double* q, int32_t K,
                   int32_t rows, int32_t cols, int32_t n_real, uint64_t seed, double* out,
                   int32_t install);
/* Device pointers, asynchronous on `stream`; d_out [max(n_real,1)][rows][cols]. */
int rhmc_gen_image_device(rhmc_ctx* ctx, const rhmc_params* P, const double* d_q, int32_t K,
                          int32_t rows, int32_t cols, int32_t n_real, uint64_t seed,
                          double* d_out, void* stream);

/*
 * samplers.lightsource_gym.find_peaks' seed descent (samplers.py:190-221):
 * every seed q[i] = (f, x, y) (counts, pixels) runs gradient descent on the
 * one-star potential V = -sum(D ln Lambda - Lambda), Lambda = B + f PSF over
 * the whole image (V_single :121-127, dVdq_single :93-101), for at most
 * n_step steps:
 *   dt_f = f dt_f_coeff, dt_xy = dt_xy_coeff / f   (from f before the update)
 *   f -= dV/df dt_f, x -= dV/dx dt_xy, y -= dV/dy dt_xy
 *   f < f_lim: RHMC_PEAK_FAINT (the state keeps the update)
 *   |(V - V_prev)/V_prev| < rel_tol: RHMC_PEAK_CONVERGED (the reference: 1e-9)
 * and RHMC_PEAK_CAP after n_step steps.  There is no other confinement.  A
 * seed whose state turns non-finite passes neither test: it ends with
 * steps = n_step and RHMC_PEAK_CAP | RHMC_STATUS_NONFINITE.  Only P->B_count
 * and P->fwhm_pix are read from P (no prior, no repulsion); f_lim is opts'.
 * q [n][3] is updated in place; steps [n] (gradient evaluations), status [n]
 * and V [n] (the last V evaluated: the initial V for a seed faint after its
 * first step) are nullable.  n = 0 is a no-op.  RHMC_ERR_ARG: NULL ctx, q or
 * opts, n < 0, n_step < 0 or > 10^6, a non-finite coefficient.
 */
typedef struct rhmc_peaks_opts {
  double f_lim;        /* flux below which a seed disappears (counts)        */
  double dt_f_coeff;   /* find_peaks' dt_f_coeff                             */
  double dt_xy_coeff;  /* find_peaks' dt_xy_coeff                            */
  double rel_tol;      /* relative change of V that ends the descent         */
  int32_t n_step;      /* find_peaks' Nstep                                  */
  int32_t reserved;    /* must be 0                                          */
} rhmc_peaks_opts;
int rhmc_find_peaks(rhmc_ctx* ctx, const rhmc_params* P, const rhmc_peaks_opts* opts, double* q,
                    int64_t n, int32_t* steps, int32_t* status, double* V);
/* Device pointers, asynchronous on `stream` (the stepwise path may wait for
 * the stream every 16 steps to stop once every seed has). */
int rhmc_find_peaks_device(rhmc_ctx* ctx, const rhmc_params* P, const rhmc_peaks_opts* opts,
                           double* d_q, int64_t n, int32_t* d_steps, int32_t* d_status,
                           double* d_V, void* stream);

/*
 * The trial of samplers.lightsource_gym.HMC_find_best_dt's step-size search
 * (samplers.py:332-371, identical at :399-438), n independent tasks.  Task t
 * starts at q0[t] = (f, x, y) with the step vector dt[t] against the
 * background image bg[bg_index[t]] (fp64, the context's image shape) and the
 * context's data image D, and runs opts->n_iter iterations i of
 *   p  = z[t][i]                    (flux_only[t] != 0: p[1] = p[2] = 0, :343-345)
 *   E0 = V(q) + (p.p)/2             V = -sum(D ln L - L), L = bg + f PSF(x, y)
 *                                   over all pixels (:121-127)
 *   ph = p - dt G(q)/2              (:352)
 *   steps[t][i] times: q = q + dt ph ; ph = ph - dt G(q)      (:354-356)
 *   p  = ph + dt G(q)/2 ; dE = V(q) + (p.p)/2 - E0
 *   accept when dE < 0 or lnu[t][i] < -dE (:366), else q returns to the
 *   iteration's start.
 * n_accept[t] counts the accepted iterations.  PSF and pixel convention as at
 * rhmc_gen_image.  opts->grad selects G: RHMC_DT_GRAD_REFERENCE is what the
 * reference's call computes, dVdq_single with its default f_only=True (:77,
 * :102-104): the flux gradient -sum (D/L - 1) PSF used for all three
 * coordinates; RHMC_DT_GRAD_FULL is the true (dV/df, dV/dx, dV/dy) (:93-101).
 * There is no flux wall and no confinement; non-finite values propagate
 * (0 * NaN stays NaN, so dt = (dt_f, 0, 0) with flux_only needs no mode of its
 * own) and end in a rejection.  A task's result depends on nothing but its own
 * inputs (not on n, its position or its batch-mates).
 *
 * Draws: z [n][n_iter][3] standard normals, steps [n][n_iter] and lnu
 * [n][n_iter] = log(u) from the host (the reference's randn(3), randint(
 * steps_min, steps_max, 1), log(random(1)) per iteration), all three or none.
 * With none the device draws them with Philox-4x32-10 under key `seed`, counter
 * (draw, iteration, stream_id[t]): draws 0 and 1 are the Box-Muller pairs of z,
 * 0x80000001 the step count, uniform on [steps_min, steps_max), 0x80000000 u in
 * (0, 1]; a task's draws depend on nothing but seed and stream_id[t].
 * stream_id is read only then; steps_min / steps_max likewise (0 <= steps_min
 * < steps_max <= 65536).
 *
 * rec (nullable, every member nullable): per iteration dE, accept, q after
 * the iteration, and the draws used (z as drawn, before flux_only zeroes it).
 * Only P->B_count and P->fwhm_pix are read from P (B_count not by the trial).
 * n = 0 is a no-op.  RHMC_ERR_ARG: NULL ctx, P, opts, bg, bg_index, q0 or dt
 * (stream_id without host draws), n < 0, n_bg < 1, n_iter outside 1..1024, an
 * unknown grad, non-zero reserved, only some of z / steps / lnu, and on the
 * host entry point bg_index outside [0, n_bg) or steps outside 0..65535 (the
 * device entry point clamps both into range instead).
 */
enum { RHMC_DT_GRAD_REFERENCE = 0, RHMC_DT_GRAD_FULL = 1 };
typedef struct rhmc_dt_opts {
  int32_t n_iter;      /* HMC_find_best_dt's Niter_per_trial, 1..1024          */
  int32_t grad;        /* RHMC_DT_GRAD_*                                       */
  int32_t steps_min;   /* device draws: steps uniform on [steps_min, steps_max) */
  int32_t steps_max;
  int32_t reserved[2]; /* must be 0                                            */
} rhmc_dt_opts;
typedef struct rhmc_dt_record {
  double* dE;          /* [n][n_iter]                                          */
  int32_t* accept;     /* [n][n_iter]                                          */
  double* q;           /* [n][n_iter][3] q after the iteration                 */
  double* z;           /* [n][n_iter][3] the draws used                        */
  int32_t* steps;      /* [n][n_iter]                                          */
  double* lnu;         /* [n][n_iter]                                          */
} rhmc_dt_record;
int rhmc_dt_trials(rhmc_ctx* ctx, const rhmc_params* P, const rhmc_dt_opts* opts,
                   const double* bg, int32_t n_bg, const int32_t* bg_index, const double* q0,
                   const double* dt, const int32_t* flux_only, int64_t n, const double* z,
                   const int32_t* steps, const double* lnu, uint64_t seed,
                   const uint64_t* stream_id, int32_t* n_accept, const rhmc_dt_record* rec);
/* Device pointers (rec itself is a host struct of device pointers),
 * asynchronous on `stream`. */
int rhmc_dt_trials_device(rhmc_ctx* ctx, const rhmc_params* P, const rhmc_dt_opts* opts,
                          const double* d_bg, int32_t n_bg, const int32_t* d_bg_index,
                          const double* d_q0, const double* d_dt, const int32_t* d_flux_only,
                          int64_t n, const double* d_z, const int32_t* d_steps,
                          const double* d_lnu, uint64_t seed, const uint64_t* d_stream_id,
                          int32_t* d_n_accept, const rhmc_dt_record* rec, void* stream);

/*
 * The whole Metropolis-Hastings chain of samplers.lightsource_gym.HMC_random
 * (RHMC_CHAIN_UNIT, samplers.py:460-572) or RHMC_random_diag (RHMC_CHAIN_DIAG,
 * :668-825) on the device: n independent chains of K stars, opts->n_iter
 * iterations, everything queued on one stream with no host round trip (per
 * iteration one launch for the decision and the next draw, one for the
 * trajectories, one for V).  q [n][3K] is updated in place to the last state.
 *
 * Row 0 (:507-513, :725-731): p = z[0] sqrt(M(q)), E_chain[0] = E(q, p),
 * dE_chain[0] = 0, q_chain[0] = q.  Iteration i = 1 .. n_iter (:516-568,
 * :738-817):
 *   p = z[i] sqrt(M(q))             UNIT: M = 1, p = z[i]; DIAG: M = (1/f,
 *                                   f factor1, f factor1) per star (:574-590)
 *   E_initial = E(q, p)             E_chain[i]; dE_chain[i] = E_chain[i] -
 *                                   E_chain[i-1] (:526, :751)
 *   (q', p') = the trajectory of rhmc_hmc_random (UNIT, step vector dt [3K]) or
 *              rhmc_diag_random (DIAG, the one step dt_global) from (q, p),
 *              steps[i][c] steps long, with their quirks: the sticky flip mask,
 *              and p' = p as it went in when the last step flipped (:549-554)
 *   E_final = E(q', p')             DIAG: with M(q') (:803-804)
 *   dE = E_final - E_initial; the chain accepts iff dE < 0 or lnu[i] < -dE
 *   (:563, :810), then q = q'; otherwise q stays.  q_chain[i] = q.
 * E(q, p) (:1152-1161) is +inf when any flux is below P->f_lim (:1157-1159),
 * else V(q) + K(p): V is what rhmc_energy gives with f_pos = RHMC_V_NO_POSCHECK
 * (no prior, no wall, no position check); UNIT: K = sum(p^2)/2 (:1171); DIAG:
 * K = (sum(p^2/M) + log|prod M|)/2 (:1173), the product a running product in
 * index order like np.prod, so that an overflowing product behaves as the
 * reference's does.  NaN compares false everywhere: a NaN chain rejects for
 * ever.  V of the current state is carried from the last accepted proposal,
 * not recomputed (the engine's V of a chain does not depend on its batch).
 *
 * Draws: z [n_iter+1][n][3K] standard normals (row 0: p_initial), steps
 * [n_iter][n] and lnu [n_iter][n] = log(u) from the host, all three or none
 * (row i - 1 of steps and lnu belongs to iteration i).  With none the device
 * draws them with Philox-4x32-10 under key `seed`, counter (draw, iter0 + i,
 * stream_id[c]): draw j/2 is the Box-Muller pair of normal j, 0x80000001 the
 * length, uniform on [steps_min, steps_max), 0x80000000 u in (0, 1]; stream_id
 * NULL means the chain index c.  A chain's result depends on nothing but its
 * own start, seed, stream_id[c] and iter0 — not on n, its position or its
 * batch-mates — so a long run can be recorded in pieces (iter0 = the number of
 * the iteration before this call's first; row 0 of a later piece is then drawn
 * with the counter of the piece before's last iteration and its E_chain[0] is
 * not the run's) and a sharded run can pass global chain numbers.
 *
 * rec (nullable, every member nullable) is iteration-major like
 * rhmc_mh_record; status holds the trajectories' RHMC_STATUS_* words, z, steps
 * and lnu the draws used.
 * RHMC_ERR_ARG, all checked before any device call: NULL ctx, P or opts; NULL
 * q with n > 0; NULL dt for UNIT; only some of z / steps / lnu; an unknown
 * metric; n_iter < 0 or iter0 < 0; reserved != 0; DIAG: a non-finite dt_global
 * or a factor1 that is non-finite or <= 0; device draws: steps_min / steps_max
 * outside 1 <= steps_min < steps_max <= 65536; host entry point with host
 * draws: any steps < 1; K outside 1..1024; n < 0 or n > 2^31.  n = 0 is a
 * no-op; n_iter = 0 writes row 0 only.  One thread per context, like
 * rhmc_diag_random.
 */
enum { RHMC_CHAIN_UNIT = 0,   /* HMC_random, samplers.py:460-572       */
       RHMC_CHAIN_DIAG = 1 }; /* RHMC_random_diag, samplers.py:668-825 */
typedef struct rhmc_chain_opts {
  double dt_global;    /* DIAG: the one step (finite); UNIT: ignored           */
  double factor1;      /* DIAG: F(f) = f factor1 (finite, > 0); UNIT: ignored  */
  int32_t metric;      /* RHMC_CHAIN_*                                         */
  int32_t n_iter;      /* Niter >= 0                                           */
  int32_t iter0;       /* >= 0: number of the iteration before this call's first */
  int32_t steps_min;   /* device draws: lengths uniform on [steps_min, steps_max), */
  int32_t steps_max;   /*   1 <= steps_min < steps_max <= 65536                */
  int32_t reserved;    /* must be 0                                            */
} rhmc_chain_opts;
typedef struct rhmc_chain_record {   /* every member nullable */
  double* q_chain;     /* [n_iter+1][n][3K] row 0 the start, row i the state after iteration i */
  double* E_chain;     /* [n_iter+1][n] E(start of iteration i, its momentum); row 0: E(q0, p_initial) */
  double* dE_chain;    /* [n_iter+1][n] row 0 = 0, row i = E_chain[i] - E_chain[i-1] */
  int32_t* accept;     /* [n_iter][n]                                          */
  int32_t* status;     /* [n_iter][n] the trajectory's status word             */
  double* z;           /* [n_iter+1][n][3K] the normals used                   */
  int32_t* steps;      /* [n_iter][n] the lengths used                         */
  double* lnu;         /* [n_iter][n]                                          */
} rhmc_chain_record;
int rhmc_chain(rhmc_ctx* ctx, const rhmc_params* P, const rhmc_chain_opts* opts, const double* dt,
               double* q, int64_t n, int32_t K, const double* z, const int32_t* steps,
               const double* lnu, uint64_t seed, const uint64_t* stream_id,
               const rhmc_chain_record* rec);
/* Device pointers (rec itself is a host struct of device pointers),
 * asynchronous on `stream`. */
int rhmc_chain_device(rhmc_ctx* ctx, const rhmc_params* P, const rhmc_chain_opts* opts,
                      const double* d_dt, double* d_q, int64_t n, int32_t K, const double* d_z,
                      const int32_t* d_steps, const double* d_lnu, uint64_t seed,
                      const uint64_t* d_stream_id, const rhmc_chain_record* rec, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* RHMC_H */
