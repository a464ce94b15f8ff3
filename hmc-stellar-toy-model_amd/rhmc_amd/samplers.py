"""The reference's older `samplers` API, routed to the MI355X engine:
`lightsource_gym` with its three-stage pipeline — `find_peaks` (seed stars),
`HMC_find_best_dt` (the step vector: the default branch and the step-size
search) and unit-mass HMC (`HMC_random`) — and its own Riemannian samplers,
`RHMC_random_diag` (leapfrog under the flux-dependent diagonal mass matrix) and
`RHMC_random` (the metric is the diagonal of the likelihood's Hessian).

Mirrors jaekor91/HMC-stellar-toy-model `samplers.py` (file:line per method):
same class name, attributes (set after construction, like the reference's
scripts: `gym.Nobjs`, `gym.d = 3 * Nobjs`, `gym.dt = <vector [d]>`), method
names, argument meaning, global-NumPy-RNG draw order and results.

What runs where:
  * dVdq, V, the HMC_random, RHMC_random_diag and RHMC_random trajectories,
    RHMC_efficient_computation's derivative sets, find_peaks' gradient descent
    of the seeds and the trials of HMC_find_best_dt's search run in librhmc.so
    (rhmc_gradient kind 0, rhmc_energy without the position check,
    rhmc_hmc_random, rhmc_diag_random, rhmc_hess_random, rhmc_hess_derivs,
    rhmc_find_peaks, rhmc_dt_trials).  No CPU fallback.
  * With engine="device", HMC_random_batched and RHMC_random_diag_batched run
    the whole MH chain — the momentum draw, E, the trajectories and the accept
    test — in one rhmc_chain call with no host round trip per iteration:
    rng="numpy" pre-draws from the global NumPy stream in the host loop's order
    (the stream ends where the host engine leaves it), rng="philox" draws on
    the device under `seed` and `stream_ids` and touches no NumPy stream.
    engine="host" (the default) is the NumPy loop below; RHMC_random stays on
    it (no restore on reject, the i % 100 stop), and so does save_traj.
  * E, K, p_sample, the MH bookkeeping, the diagonal metric's host methods
    (compute_factors, mass_matrix, F, G, dlnDetdq, dpMpdq), find_peaks' seed
    grid and its merge of near-duplicate peaks (merge_peaks), and everything
    between the trials of the search (the coarse ladder, the bisection, the
    per-star Poisson realisation) stay on the host (NumPy), like the reference.

Quirks kept on purpose (samplers.py:519-552): the flux-wall flip mask is
never cleared inside a trajectory, and a trajectory whose last step flipped
is evaluated with the momentum it started from.  HMC_random requires
Nchain == 1 (assert, like the reference); HMC_random_batched runs many chains
at once and, with one chain, draws exactly what HMC_random draws.

HMC_find_best_dt's step-size search (default=False, samplers.py:306-456)
takes one more keyword than the reference's call: rng="numpy" runs the
reference draw for draw from the global NumPy stream (one rhmc_dt_trials call
per trial), rng="philox" searches all stars at once with the device's draws
(one call per round of trials).  Without rng the call raises
NotImplementedError, as before the search existed.

RHMC_random_diag (samplers.py:668-825) keeps its quirks too: dpMpdq is
evaluated with the momentum the iteration started with on every step, the flip
mask is sticky, a trajectory whose last step flipped keeps its starting
momentum, and K's log-determinant is the log of a running product.  It
requires Nchain == 1 like the reference; RHMC_random_diag_batched runs many
chains at once and, with one chain, draws exactly what RHMC_random_diag draws.
factor1 is computed on first use when compute_factors() has not been called.
With save_traj, qs comes from the kernel's trace, Vs from one batched energy
call per iteration and Ts from the host.
RHMC_random (samplers.py:930-1105) and RHMC_efficient_computation (:828-927)
keep theirs: dVdqq is the mass matrix as it comes (negative or zero included);
the position flags are set for every coordinate below the image side, so px
and py of a star inside the image are negated on every step; the loop runs
i = 0 .. Niter and draws a momentum in every pass; a rejected proposal is NOT
restored (q_chain[i] is the trajectory's end state either way) and the
caller's float64 q_model_0 is overwritten; the run stops at i % 100 == 0 below
50% acceptance and leaves the later rows zero.  It serves 1 <= K <= 16 on
square images of side 16..48 (RhmcError RHMC_ERR_UNSUPPORTED otherwise) and
f_lim >= 0; debug=True is accepted and prints nothing.  RHMC_random_batched
runs many chains at once; with one chain its chains equal RHMC_random's and
only the NumPy stream's position after an early stop differs.
Out of scope: the GMM testbed (RHMC_GMM) and the plots.
"""
import numpy as np

from . import capi
from .photometry import (default_exp_setup, factors, flux2mag, gauss_PSF, mag2flux,
                         poisson_realization)


def seed_grid(num_rows, num_cols, linear_pix_density, f_seed):
    """samplers.py:168-180: the jittered grid of seeds [Nobjs_tot, 3], two
    np.random.randn() draws per seed in the reference's order and its index
    idx = i * Nobjs_row + j."""
    Nobjs_row = int(linear_pix_density * num_rows) - 1
    Nobjs_col = int(linear_pix_density * num_cols) - 1
    grid_spacing = 1 / float(linear_pix_density)
    q_seed = np.zeros((Nobjs_row * Nobjs_col, 3), dtype=float)
    for i in range(Nobjs_row):
        for j in range(Nobjs_col):
            idx = i * Nobjs_row + j
            x = grid_spacing * (i + 0.5 + 0.1 * np.random.randn())
            y = grid_spacing * (j + 0.5 + 0.1 * np.random.randn())
            q_seed[idx] = np.array([f_seed, x, y])
    return q_seed


def merge_peaks(q_seed, flux_to_count, dr_tol=1., dmag_tol=0.5):
    """samplers.py:232-252: the sequential merge of near-duplicate peaks.  The
    first remaining peak is kept and every later one within dr_tol pixels AND
    dmag_tol magnitudes of it is dropped, until none remains.  q_seed [n, 3]
    with n >= 1; returns the kept peaks [m, 3] in order."""
    q_seed = np.asarray(q_seed, dtype=float).reshape(-1, 3)
    final = []
    while True:
        q_ref = q_seed[0]
        final.append(q_ref)
        q_seed = q_seed[1:, :]
        dist_sq = (q_seed[:, 1] - q_ref[1]) ** 2 + (q_seed[:, 2] - q_ref[2]) ** 2
        with np.errstate(invalid="ignore", divide="ignore"):
            mag_seed = flux2mag(q_seed[:, 0] / flux_to_count)
            mag_ref = flux2mag(q_ref[0] / flux_to_count)
            ibool = np.logical_or(dist_sq > dr_tol ** 2, np.abs(mag_ref - mag_seed) > dmag_tol)
        q_seed = q_seed[ibool]
        if q_seed.shape[0] == 0:
            break
    return np.vstack(final)


DT_COARSE_CAP = 64      # trials of one coarse loop before the search gives up


def dt_stream_id(star, phase, stage, trial):
    """The Philox stream of one trial of HMC_find_best_dt(rng="philox"):
    star << 32 | phase << 31 | stage << 30 | trial, with phase 0 = flux, 1 = xy
    (samplers.py:317), stage 0 = coarse (:330), 1 = fine (:390), and trial the
    0-based number of the trial inside its loop (< 2^30)."""
    assert 0 <= trial < (1 << 30) and 0 <= star < (1 << 32)
    return (int(star) << 32) | (int(phase) << 31) | (int(stage) << 30) | int(trial)


def dt_star_search(star, f0, Niter_per_trial, Ntrial, dt_f_coeff, dt_xy_coeff, A_target_f,
                   A_target_xy):
    """samplers.py:309-456 for one star as a generator: everything between
    the trials, in the reference's NumPy expressions.  Yields (phase, stage,
    trial number, dt [3]) for the trial to run next and is sent the number of
    accepted iterations; returns (dt_f, dt_xy)."""
    dt_xy = dt_xy_coeff / f0
    dt_f = dt_f_coeff * f0
    for k in range(2):
        if k == 0:
            dt = np.array([dt_f, 0, 0])
            A_target = A_target_f
        else:
            dt = np.array([dt_f, dt_xy, dt_xy])
            A_target = A_target_xy
        n_coarse = 0
        while True:                                           # :330
            if n_coarse == DT_COARSE_CAP:
                raise RuntimeError("HMC_find_best_dt: star %d did not reach the target "
                                   "acceptance in %d coarse trials" % (star, DT_COARSE_CAP))
            A_rate = (yield k, 0, n_coarse, dt.copy())
            n_coarse += 1
            A_rate /= float(Niter_per_trial)                  # :371
            if A_rate < A_target:                             # :374-378
                if k == 0:
                    dt /= 10.
                else:
                    dt[1:] = dt[1:] / 10.
            else:
                break
        counter = 0                                           # :383-387
        dt_left = dt
        dt_right = 10. * dt
        if k == 1:
            dt_right[0] = dt_f
        while counter < Ntrial:                               # :390
            counter += 1
            dt = (dt_left + dt_right) / 2.                    # :394
            if k == 1:
                dt[0] = dt_f
            A_rate = (yield k, 1, counter - 1, dt.copy())
            A_rate /= float(Niter_per_trial)                  # :438
            if np.abs(A_rate - A_target) < 1e-2:              # :441-446
                break
            elif A_rate > A_target:
                dt_left = dt
            else:
                dt_right = dt
        if k == 0:                                            # :450-453
            dt_f = dt[0]
        else:
            dt_xy = dt[1] * 10
    return dt_f, dt_xy


class lightsource_gym(object):
    """samplers.py:3-43."""

    def __init__(self):
        self._D = None
        self._ctx = None
        self._ctx_shape = None
        self.M = None
        (self.num_rows, self.num_cols, self.flux_to_count, self.PSF_FWHM_pix,
         self.B_count, self.arcsec_to_pix, self.mB, _) = default_exp_setup()
        self.Nchain = None
        self.Niter = None
        self.thin_rate = None
        self.Nwarmup = None
        self.q_chain = None
        self.p_chain = None
        self.V_chain = None
        self.E_chain = None
        self.dE_chain = None
        self.A_chain = None
        self.dt = None           # per-coordinate step vector [d]
        self.Nobjs = None
        self.d = None
        self.f_lim = 0.
        self.factor0 = self.factor1 = self.factor2 = None   # compute_factors()
        self.q_seed = None
        self.peak_steps = None   # find_peaks diagnostics, per grid seed (pre-merge)
        self.peak_status = None
        self.device = 0

    # ---------------------------------------------------------------- data
    @property
    def D(self):
        return self._D

    @D.setter
    def D(self, value):
        self._D = None if value is None else np.ascontiguousarray(value, dtype=np.float64)
        self._ctx_shape = None

    def _context(self):
        if self._D is None:
            raise ValueError("no data image: call gen_mock_data() or set .D first")
        if self._D.shape != (self.num_rows, self.num_cols):
            raise ValueError("D has shape %s but num_rows/num_cols are %d/%d"
                             % (self._D.shape, self.num_rows, self.num_cols))
        if self._ctx is None:
            self._ctx = capi.Context(self._D, device=self.device)
        elif self._ctx_shape is None:
            self._ctx.set_image(self._D)
        self._ctx_shape = self._D.shape
        return self._ctx

    def _params(self, dt=1.0):
        # Only B, the PSF width and f_lim are read by the kernels used here;
        # the metric constants are placeholders (unit metric).
        return capi.make_params(
            dt=dt, delta=1e-6, counter_max=1000, B_count=self.B_count, f_lim=self.f_lim,
            f_low=mag2flux(self.mB + 2) * self.flux_to_count, fwhm_pix=self.PSF_FWHM_pix,
            g_xx=1., g_ff=1., g_ff2=1., g0=1., g1=1., g2=1., use_prior=False, alpha=2.,
            use_Vc=False, beta=1., Vc_r_pow=1., V_prior_const=0.)

    def gen_mock_data(self, q_true=None, return_data=False):
        """samplers.py:44-67: q_true (Nobjs, 3) = (f counts, x, y); the global
        NumPy RNG draws the Poisson realisation (bit-identical data)."""
        data = np.ones((self.num_rows, self.num_cols), dtype=float) * self.B_count
        for i in range(q_true.shape[0]):
            f, x, y = q_true[i]
            data += f * gauss_PSF(self.num_rows, self.num_cols, x, y, FWHM=self.PSF_FWHM_pix)
        data = poisson_realization(data)
        if return_data:
            return data
        self.D = data

    # ------------------------------------------------------------ potential
    def dVdq(self, objs_flat):
        """samplers.py:1108-1135 on the GPU (rhmc_gradient kind 0)."""
        return self._context().gradient(self._params(), objs_flat, kind=0)

    def V(self, objs_flat):
        """samplers.py:1137-1150 on the GPU: -sum(D ln Lambda - Lambda), no
        prior, no position check."""
        return self._context().energy(self._params(), objs_flat, None, f_pos=False,
                                      pos_check=False)[0]

    def E(self, q, p, mass_matrix=None):
        """samplers.py:1152-1161."""
        Nobjs = q.size // 3
        for l in range(Nobjs):
            if q[3 * l] < self.f_lim:
                return np.inf
        return self.V(q) + self.K(p, mass_matrix)

    def K(self, p, mass_matrix=None):
        """samplers.py:1163-1175."""
        if mass_matrix is None:
            return np.dot(p, p) / 2.
        return (np.sum(p ** 2 / mass_matrix) + np.log(np.abs(np.prod(mass_matrix)))) / 2.

    def p_sample(self):
        """samplers.py:1177-1181."""
        return np.random.randn(self.d)

    def leap_frog(self, p_old, q_old, dt):
        """samplers.py:1183-1191."""
        p_half = p_old - dt * self.dVdq(q_old) / 2.
        q_new = q_old + dt * p_half
        p_new = p_half - dt * self.dVdq(q_new) / 2.
        return p_new, q_new

    # ---------------------------------------------------------------- seeds
    def find_peaks(self, linear_pix_density=0.2, dr_tol=1., dmag_tol=0.5, mag_lim=None,
                   Nstep=1000, dt_f_coeff=1e-1, dt_xy_coeff=1e-1, no_perturb=False):
        """samplers.py:129-254.  Seeds on a jittered grid (the global NumPy RNG
        draws the jitter), each run through up to Nstep steps of gradient
        descent on the one-star potential against the pure-background model
        (on the GPU, rhmc_find_peaks); seeds that turn fainter than the limit
        disappear, near-duplicates are merged.  Sets q_seed [n, 3]; peak_steps
        / peak_status keep the per-seed step counts and capi.PEAK_* words."""
        if self.num_rows is None or self.D is None:
            print("The image must be specified first.")
            assert False
        if mag_lim is None:
            mag_lim = self.mB - 1.
        f_lim = mag2flux(mag_lim) * self.flux_to_count
        f_seed = mag2flux(mag_lim - 0.5) * self.flux_to_count
        q_seed = seed_grid(self.num_rows, self.num_cols, linear_pix_density, f_seed)
        if no_perturb:
            self.q_seed = q_seed
            return
        opts = capi.make_peaks_opts(f_lim, n_step=Nstep, dt_f_coeff=dt_f_coeff,
                                    dt_xy_coeff=dt_xy_coeff, rel_tol=1e-9)
        q_seed, steps, status, _ = self._context().find_peaks(self._params(), opts, q_seed)
        self.peak_steps = steps
        self.peak_status = status
        q_seed = q_seed[(status & capi.PEAK_FAINT) == 0]
        if q_seed.shape[0] == 0:
            self.q_seed = q_seed
            print("No peaks were found.")
            return
        self.q_seed = merge_peaks(q_seed, self.flux_to_count, dr_tol, dmag_tol)

    def HMC_find_best_dt(self, q_model_0=None, steps_min=10, steps_max=50, Niter_per_trial=10,
                         Ntrial=10, dt_f_coeff=1., dt_xy_coeff=10., default=False,
                         A_target_f=0.9, A_target_xy=0.5, rng=None, grad="reference", seed=0):
        """samplers.py:257-456: Nobjs, d and the step vector dt.  default=True:
        dt = (dt_f_coeff f, dt_xy_coeff / f, dt_xy_coeff / f) per star (:295-303).
        default=False is the step-size search (:306-456), its trials on the GPU
        (rhmc_dt_trials) and `rng` (which the reference's call does not have)
        saying where the draws come from:
          rng="numpy"   the reference draw for draw from the global NumPy
                        stream: per star the Poisson realisation, per trial
                        randn(3), randint(steps_min, steps_max, 1), random(1)
                        for each iteration, then one call with one task;
          rng="philox"  all stars at once: the Nobjs realisations first, in star
                        order, from the global stream; then every star walks its
                        own coarse / fine search and each round is one call over
                        the stars that still have a trial to run, with the
                        device's Philox draws under `seed` and the stream
                        dt_stream_id(star, phase, stage, trial);
          rng=None      NotImplementedError.
        grad="reference" uses the flux gradient for all three coordinates, as
        the reference's call does (dVdq_single's default f_only=True),
        grad="full" the true gradient.  A coarse loop that has not reached its
        target after 64 trials raises RuntimeError naming the star (the
        reference would loop forever, e.g. when V(q0) is NaN)."""
        if q_model_0 is None:
            print("Use found seeds for inference.")
            q_model_0 = self.q_seed
        q_model_0 = np.asarray(q_model_0, dtype=float).reshape(-1, 3)
        self.Nobjs = q_model_0.shape[0]
        self.d = self.Nobjs * 3
        self.dt = np.zeros(self.d)
        if default:
            for i in range(self.Nobjs):
                f0, x0, y0 = q_model_0[i]
                dt_xy = dt_xy_coeff / f0
                dt_f = dt_f_coeff * f0
                self.dt[3 * i:3 * i + 3] = np.array([dt_f, dt_xy, dt_xy])
            return
        if rng is None:
            raise NotImplementedError(
                "HMC_find_best_dt(default=False): the step-size search perturbs one star "
                "against the residual image of the others as its background, and the "
                "kernels take a constant background B; use default=True, or name the "
                "source of the search's draws: rng=\"numpy\" (the reference's stream) or "
                "rng=\"philox\" (all stars at once, rhmc_dt_trials)")
        if rng not in ("numpy", "philox"):
            raise ValueError("rng must be None, \"numpy\" or \"philox\"")
        kw = dict(steps_min=steps_min, steps_max=steps_max, Niter_per_trial=Niter_per_trial,
                  Ntrial=Ntrial, dt_f_coeff=dt_f_coeff, dt_xy_coeff=dt_xy_coeff,
                  A_target_f=A_target_f, A_target_xy=A_target_xy, grad=grad)
        if rng == "numpy":
            for l in range(self.Nobjs):
                bg = self._dt_background(q_model_0, l)
                self.dt[3 * l:3 * l + 3] = self._dt_search_numpy(q_model_0[l], l, bg, **kw)
            return
        bgs = np.stack([self._dt_background(q_model_0, l) for l in range(self.Nobjs)])
        res = self.dt_search_philox(q_model_0, bgs, range(self.Nobjs), seed=seed, **kw)
        for l in range(self.Nobjs):
            self.dt[3 * l:3 * l + 3] = res[l]

    def _dt_background(self, q_model_0, l):
        """samplers.py:314-315: a Poisson realisation of the model of all the
        stars (global NumPy stream) minus star l."""
        f0, x0, y0 = q_model_0[l]
        model_data = self.gen_mock_data(q_model_0, return_data=True)
        model_data -= f0 * gauss_PSF(self.num_rows, self.num_cols, x0, y0,
                                     FWHM=self.PSF_FWHM_pix)
        return model_data

    def _dt_search_numpy(self, q0, l, bg, steps_min, steps_max, Niter_per_trial, Ntrial,
                         dt_f_coeff, dt_xy_coeff, A_target_f, A_target_xy, grad):
        ctx, P = self._context(), self._params()
        opts = capi.make_dt_opts(Niter_per_trial, grad, steps_min, steps_max)
        gen = dt_star_search(l, q0[0], Niter_per_trial, Ntrial, dt_f_coeff, dt_xy_coeff,
                             A_target_f, A_target_xy)
        n = Niter_per_trial
        z, steps, lnu = np.zeros((n, 3)), np.zeros(n, np.int32), np.zeros(n)
        req = next(gen)
        while True:
            k, _, _, dt = req
            for i in range(n):                                # :343, :351, :365
                z[i] = np.random.randn(3)
                steps[i] = np.random.randint(low=steps_min, high=steps_max, size=1)[0]
                lnu[i] = np.log(np.random.random(1))[0]
            n_acc = ctx.dt_trials(P, opts, bg, [0], q0, dt, flux_only=[k == 0], z=z,
                                  steps=steps, lnu=lnu)
            try:
                req = gen.send(int(n_acc[0]))
            except StopIteration as e:
                dt_f, dt_xy = e.value
                return np.array([dt_f, dt_xy, dt_xy])         # :456

    def dt_search_philox(self, q_model_0, bgs, stars, steps_min=10, steps_max=50,
                         Niter_per_trial=10, Ntrial=10, dt_f_coeff=1., dt_xy_coeff=10.,
                         A_target_f=0.9, A_target_xy=0.5, grad="reference", seed=0):
        """The search of HMC_find_best_dt(rng="philox") for the stars `stars`
        of q_model_0 against their backgrounds bgs[star]: {star: step vector
        [3]}.  A star's result does not depend on which other stars are
        searched with it."""
        q_model_0 = np.asarray(q_model_0, dtype=float).reshape(-1, 3)
        ctx, P = self._context(), self._params()
        opts = capi.make_dt_opts(Niter_per_trial, grad, steps_min, steps_max)
        gens, req, out = {}, {}, {}
        for l in stars:
            gens[l] = dt_star_search(l, q_model_0[l, 0], Niter_per_trial, Ntrial, dt_f_coeff,
                                     dt_xy_coeff, A_target_f, A_target_xy)
            req[l] = next(gens[l])
        while req:
            act = sorted(req)
            n_acc = ctx.dt_trials(
                P, opts, bgs, act, q_model_0[act], [req[l][3] for l in act],
                flux_only=[req[l][0] == 0 for l in act], seed=seed,
                stream_id=[dt_stream_id(l, *req[l][:3]) for l in act])
            for l, a in zip(act, n_acc):
                try:
                    req[l] = gens[l].send(int(a))
                except StopIteration as e:
                    del req[l]
                    dt_f, dt_xy = e.value
                    out[l] = np.array([dt_f, dt_xy, dt_xy])
        return out

    # ------------------------------------------------------------- sampling
    def _trajectories(self, q, p, steps):
        """Batched samplers.py:519-552 on the GPU (rhmc_hmc_random)."""
        dt = np.ascontiguousarray(np.broadcast_to(np.asarray(self.dt, np.float64), (self.d,)))
        return self._context().hmc_random(self._params(), dt, q, p,
                                          np.asarray(steps, np.int32))

    def _set_f_lim(self, f_lim, f_lim_default):
        if f_lim_default:
            self.f_lim = mag2flux(self.mB - 1.) * self.flux_to_count
        else:
            self.f_lim = f_lim

    def HMC_random(self, q_model_0=None, Nchain=1, Niter=1000, thin_rate=0, Nwarmup=0,
                   steps_min=10, steps_max=50, f_lim=0., f_lim_default=False):
        """samplers.py:460-572.  Sets q_chain [1, Niter+1, d], E_chain,
        dE_chain [1, Niter+1, 1] and A_chain [1, Niter, 1]."""
        assert Nchain == 1  # Currently we do not support any other.
        self.Nchain = Nchain
        self.Niter = Niter
        self.thin_rate = thin_rate
        self.Nwarmup = Nwarmup
        assert self.d is not None
        self._set_f_lim(f_lim, f_lim_default)
        if q_model_0 is None:
            print("Use found seeds for inference.")
            q_model_0 = self.q_seed
        q_model_0 = np.asarray(q_model_0, dtype=float).reshape((self.d,))
        self._run(q_model_0[None, :], Niter, steps_min, steps_max)
        print("Chain %d Acceptance rate: %.2f%%"
              % (0, np.sum(self.A_chain[0, :] * 100) / float(self.Niter)))

    def HMC_random_batched(self, q_model_0, Niter=1000, steps_min=10, steps_max=50, f_lim=0.,
                           f_lim_default=False, engine="host", rng="numpy", seed=0,
                           stream_ids=None):
        """HMC_random over many independent chains at once (q_model_0
        [Nchain, d]); per iteration the global NumPy RNG draws randn(Nchain, d),
        randint(steps_min, steps_max, Nchain) and random(Nchain) — with one
        chain exactly the reference's draws.  engine="device" runs the whole
        loop in one rhmc_chain call: rng="numpy" on the same draws, taken from
        the global stream in the same order before the call; rng="philox" on
        the device's draws under `seed`, chain c on the stream stream_ids[c]
        (None: c), which touch no NumPy stream."""
        assert self.d is not None
        self._check_engine(engine, rng)
        self._set_f_lim(f_lim, f_lim_default)
        q0 = np.asarray(q_model_0, dtype=float).reshape(-1, self.d)
        self.Nchain = q0.shape[0]
        self.Niter = Niter
        if engine == "device":
            self._run_device(q0, Niter, steps_min, steps_max, "unit", 0., rng, seed, stream_ids)
        else:
            self._run(q0, Niter, steps_min, steps_max)

    @staticmethod
    def _check_engine(engine, rng):
        if engine not in ("host", "device"):
            raise ValueError("engine must be \"host\" or \"device\"")
        if rng not in ("numpy", "philox"):
            raise ValueError("rng must be \"numpy\" or \"philox\"")
        if engine == "host" and rng == "philox":
            raise ValueError("rng=\"philox\" draws on the device: it needs engine=\"device\"")

    def _run_device(self, q0, Niter, steps_min, steps_max, metric, dt_global, rng, seed,
                    stream_ids):
        """The MH loop of _run (metric "unit") or _run_diag ("diag") in one
        rhmc_chain call, its iteration-major records transposed into the
        reference's [Nchain, Niter(+1), .] shapes."""
        ctx, P = self._context(), self._params()
        n, d = q0.shape
        z = steps = lnu = None
        if rng == "numpy":                                    # the host loop's order
            z = np.empty((Niter + 1, n, d))
            steps = np.empty((Niter, n), np.int32)
            lnu = np.empty((Niter, n))
            z[0] = np.random.randn(n, d)
            for i in range(Niter):
                z[i + 1] = np.random.randn(n, d)
                steps[i] = np.random.randint(low=steps_min, high=steps_max, size=n)
                lnu[i] = np.log(np.random.random(n))
        diag = metric == "diag"
        opts = capi.make_chain_opts(metric, Niter, dt_global=dt_global,
                                    factor1=self.factor1 if diag else 0., steps_min=steps_min,
                                    steps_max=steps_max)
        dt = None if diag else np.ascontiguousarray(
            np.broadcast_to(np.asarray(self.dt, np.float64), (d,)))
        out = ctx.chain(P, opts, q0, dt=dt, z=z, steps=steps, lnu=lnu, seed=seed,
                        stream_id=None if rng == "numpy" else stream_ids,
                        record=("q_chain", "E_chain", "dE_chain", "accept"))
        self.q_chain = np.ascontiguousarray(np.transpose(out["q_chain"], (1, 0, 2)))
        self.E_chain = np.ascontiguousarray(out["E_chain"].T)[:, :, None]
        self.dE_chain = np.ascontiguousarray(out["dE_chain"].T)[:, :, None]
        self.A_chain = np.ascontiguousarray(out["accept"].T).astype(float)[:, :, None]

    def _E_batch(self, q, p):
        V = self._context().energy(self._params(), q, None, f_pos=False, pos_check=False)[0]
        E = V + np.sum(p * p, axis=1) / 2.
        E[(q[:, 0::3] < self.f_lim).any(axis=1)] = np.inf
        return E

    # ------------------------------------------- the diagonal-metric sampler
    def compute_factors(self):
        """samplers.py:69-75."""
        self.factor0, self.factor1, self.factor2 = factors(
            self.num_rows, self.num_cols, self.num_rows / 2., self.num_cols / 2.,
            self.PSF_FWHM_pix)

    def F(self, f, dFdf=False):
        """samplers.py:592-600."""
        x1 = f * self.factor1
        return (x1, self.factor1) if dFdf else x1

    def G(self, f, dGdf=False):
        """samplers.py:614-625."""
        x1 = 1. / f
        return (x1, -1 / f ** 2) if dGdf else x1

    def mass_matrix(self, q):
        """samplers.py:574-590: M = diag(G(f), F(f), F(f)) per star, q [d]."""
        M = np.zeros_like(q)
        for i in range(int(q.shape[0]) // 3):
            f = q[3 * i]
            M[3 * i] = self.G(f)
            M[(3 * i) + 1:3 * (i + 1)] = self.F(f)
        return M

    def dlnDetdq(self, q):
        """samplers.py:636-649."""
        out = np.zeros_like(q)
        for i in range(int(q.shape[0]) // 3):
            f = q[3 * i]
            G, dGdf = self.G(f, dGdf=True)
            F, dFdf = self.F(f, dFdf=True)
            out[3 * i] = 0.5 * (dGdf / G + 2 * dFdf / F)
        return out

    def dpMpdq(self, q, p):
        """samplers.py:651-664."""
        out = np.zeros_like(q)
        for i in range(int(q.shape[0]) // 3):
            f = q[3 * i]
            pf, px, py = p[3 * i:3 * (i + 1)]
            G, dGdf = self.G(f, dGdf=True)
            F, dFdf = self.F(f, dFdf=True)
            out[3 * i] = - 0.5 * (dGdf * pf ** 2 / G ** 2 + (px ** 2 + py ** 2) * dFdf / F ** 2)
        return out

    def _mass_batch(self, q):
        """mass_matrix over chains q [n, d]."""
        M = np.empty_like(q)
        f = q[:, 0::3]
        with np.errstate(all="ignore"):
            M[:, 0::3] = 1. / f
            M[:, 1::3] = M[:, 2::3] = f * self.factor1
        return M

    def _K_batch(self, p, M):
        """K(p, M) per chain: a running product, then one log, like the
        reference (an overflowing product behaves as its does)."""
        with np.errstate(all="ignore"):
            return (np.sum(p ** 2 / M, axis=1) + np.log(np.abs(np.prod(M, axis=1)))) / 2.

    def _E_diag_batch(self, q, p, M):
        V = self._context().energy(self._params(), q, None, f_pos=False, pos_check=False)[0]
        E = V + self._K_batch(p, M)
        E[(q[:, 0::3] < self.f_lim).any(axis=1)] = np.inf
        return E

    def RHMC_random_diag(self, q_model_0, Nchain=1, Niter=1000, thin_rate=0, Nwarmup=0,
                         steps_min=10, steps_max=50, f_lim=0., f_lim_default=False,
                         dt_global=1e-2, save_traj=False):
        """samplers.py:668-825: leapfrog under the flux-dependent diagonal mass
        matrix with the one step dt_global, the trajectories on the GPU
        (rhmc_diag_random).  q_model_0 (Nobjs, 3).  Sets Nobjs, d, q_chain
        [1, Niter+1, d], E_chain, dE_chain [1, Niter+1, 1] and A_chain [1,
        Niter, 1]; with save_traj the lists qs, Vs, Ts (entry 0 the start, then
        per iteration q, V(q) and K(p_start, M(q)) after every step)."""
        assert Nchain == 1  # Currently we do not support any other.
        self.Nchain = Nchain
        self.Niter = Niter
        self.thin_rate = thin_rate
        self.Nwarmup = Nwarmup
        self._set_f_lim(f_lim, f_lim_default)
        if q_model_0 is None:
            print("Use found seeds for inference.")
            q_model_0 = self.q_seed
        q_model_0 = np.asarray(q_model_0, dtype=float)
        self.Nobjs = q_model_0.shape[0]
        self.d = int(np.prod(q_model_0.shape))
        self._run_diag(q_model_0.reshape((1, self.d)), Niter, steps_min, steps_max, dt_global,
                       save_traj)
        print("Chain %d Acceptance rate: %.2f%%"
              % (0, np.sum(self.A_chain[0, :] * 100) / float(self.Niter)))

    def RHMC_random_diag_batched(self, q_model_0, Niter=1000, steps_min=10, steps_max=50,
                                 f_lim=0., f_lim_default=False, dt_global=1e-2, engine="host",
                                 rng="numpy", seed=0, stream_ids=None):
        """RHMC_random_diag over many independent chains at once (q_model_0
        [Nchain, d]); per iteration the global NumPy RNG draws randn(Nchain, d),
        randint(steps_min, steps_max, Nchain) and random(Nchain) — with one
        chain exactly the reference's draws.  engine / rng / seed / stream_ids
        as in HMC_random_batched."""
        self._check_engine(engine, rng)
        self._set_f_lim(f_lim, f_lim_default)
        q0 = np.asarray(q_model_0, dtype=float)
        q0 = q0.reshape(1, -1) if q0.ndim == 1 else q0.reshape(q0.shape[0], -1)
        self.Nchain, self.d = q0.shape
        self.Nobjs = self.d // 3
        self.Niter = Niter
        if engine == "device":
            if getattr(self, "factor1", None) is None:
                self.compute_factors()
            self._run_device(q0, Niter, steps_min, steps_max, "diag", dt_global, rng, seed,
                             stream_ids)
        else:
            self._run_diag(q0, Niter, steps_min, steps_max, dt_global, False)

    def _run_diag(self, q0, Niter, steps_min, steps_max, dt_global, save_traj):
        if getattr(self, "factor1", None) is None:
            self.compute_factors()
        ctx, P = self._context(), self._params()
        n, d = q0.shape
        self.q_chain = np.zeros((n, Niter + 1, d))
        self.E_chain = np.zeros((n, Niter + 1, 1))
        self.dE_chain = np.zeros((n, Niter + 1, 1))
        self.A_chain = np.zeros((n, Niter, 1))
        self.q_chain[:, 0, :] = q0
        M = self._mass_batch(q0)
        with np.errstate(all="ignore"):
            p_initial = np.random.randn(n, d) * np.sqrt(M)
        self.E_chain[:, 0, 0] = self._E_diag_batch(q0, p_initial, M)
        E_previous = self.E_chain[:, 0, 0].copy()
        q_tmp = q0.copy()
        if save_traj:                                         # :734-737 (one chain)
            self.qs = [np.array([q0[0]])]
            self.Vs = [np.array([self.V(q0[0])])]
            self.Ts = [self._K_batch(p_initial, M)]
        for i in range(1, Niter + 1):
            q_initial = q_tmp
            M = self._mass_batch(q_initial)
            with np.errstate(all="ignore"):
                p_tmp = np.random.randn(n, d) * np.sqrt(M)
            E_initial = self._E_diag_batch(q_tmp, p_tmp, M)
            self.E_chain[:, i, 0] = E_initial
            with np.errstate(invalid="ignore"):
                self.dE_chain[:, i, 0] = E_initial - E_previous
            steps = np.random.randint(low=steps_min, high=steps_max, size=n)
            if save_traj:
                q_new, p_new, trace = ctx.diag_random(P, dt_global, self.factor1, q_tmp, p_tmp,
                                                      steps, trace=True)
                qs = trace[0, :steps[0] + 1]
                self.qs.append(qs)                            # one batched V per iteration
                self.Vs.append(ctx.energy(P, qs, None, f_pos=False, pos_check=False)[0])
                # the stale-momentum quirk: K of the START momentum at every q (:790)
                self.Ts.append(self._K_batch(np.broadcast_to(p_tmp[0], qs.shape),
                                             self._mass_batch(qs)))
            else:
                q_new, p_new = ctx.diag_random(P, dt_global, self.factor1, q_tmp, p_tmp, steps)
            E_final = self._E_diag_batch(q_new, p_new, self._mass_batch(q_new))
            with np.errstate(invalid="ignore"):
                dE = E_final - E_initial
            E_previous = E_initial
            lnu = np.log(np.random.random(n))
            with np.errstate(invalid="ignore"):
                acc = (dE < 0) | (lnu < -dE)
            self.A_chain[:, i - 1, 0] = acc
            q_tmp = np.where(acc[:, None], q_new, q_initial)
            self.q_chain[:, i, :] = q_tmp

    # ------------------------------------------- the Hessian-metric sampler
    def RHMC_efficient_computation(self, q_tmp, p_tmp, debug=True, dVdqq_only=False):
        """samplers.py:828-927 with the reference's three return shapes:
        dVdqq [d] with dVdqq_only (no wall check); (inf, inf, inf) when a flux
        is below f_lim; else (dqdt, dpdt, E).  The derivative sums and V come
        from the GPU (rhmc_hess_derivs).  debug is accepted and prints
        nothing (the reference dumps every intermediate)."""
        q_tmp = np.asarray(q_tmp, dtype=float).reshape(-1)
        if not dVdqq_only and (q_tmp[0::3] < self.f_lim).any():
            return np.inf, np.inf, np.inf
        dVdq, dVdqq, dVdqqq, V = self._context().hess_derivs(self._params(), q_tmp, V=True)
        if dVdqq_only:
            return dVdqq
        with np.errstate(all="ignore"):
            dqdt = p_tmp / dVdqq
            dpdt = -dVdqqq * ((1. / dVdqq) - dqdt ** 2) / 2. - dVdq
            K = np.sum((p_tmp ** 2) / dVdqq) / 2. + np.log(np.prod(dVdqq)) / 2.
            E = K + V
        return dqdt, dpdt, E

    def _E_hess_batch(self, q, p, dVdqq, V):
        """E of RHMC_efficient_computation per chain: inf below the wall, else
        K + V with K's log-determinant the log of a running product."""
        with np.errstate(all="ignore"):
            E = np.sum(p ** 2 / dVdqq, axis=1) / 2. + np.log(np.prod(dVdqq, axis=1)) / 2. + V
        E[(q[:, 0::3] < self.f_lim).any(axis=1)] = np.inf
        return E

    def RHMC_random(self, q_model_0=None, Nchain=1, Niter=1000, thin_rate=0, Nwarmup=0,
                    steps_min=10, steps_max=50, f_lim=0., f_lim_default=False, dt_RHMC_xy=1.,
                    dt_RHMC_f=0.1, debug=True):
        """samplers.py:930-1105: leapfrog under the metric diag(dVdqq), the
        diagonal of the likelihood's Hessian, the trajectories on the GPU
        (rhmc_hess_random).  q_model_0 (Nobjs, 3).  Sets Nobjs, d, q_chain
        [1, Niter+1, d], E_chain, dE_chain [1, Niter+1, 1], A_chain [1, Niter,
        1] and R_accept.  Like the reference: the loop runs i = 0 .. Niter and
        draws a momentum in every pass; a rejected proposal is NOT restored
        (q_chain[i] is the trajectory's end state either way) and a float64
        q_model_0 is overwritten with the last state; "Divergence encountered
        at (i ,z)" is printed when a trajectory breaks off; at every i % 100 ==
        0 the run stops when fewer than 50% were accepted so far (later rows
        stay zero).  debug is accepted and prints nothing.  f_lim < 0 is
        refused by the library."""
        assert Nchain == 1  # Currently we do not support any other.
        self.Nchain = Nchain
        self.Niter = Niter
        self.thin_rate = thin_rate
        self.Nwarmup = Nwarmup
        if q_model_0 is None:
            print("Use found seeds for inference.")
            q_model_0 = self.q_seed
        q_model_0 = np.asarray(q_model_0, dtype=float)
        self.Nobjs = q_model_0.shape[0]
        self.d = self.Nobjs * 3
        self._set_f_lim(f_lim, f_lim_default)
        self._run_hess(q_model_0.reshape((1, self.d)), Niter, steps_min, steps_max, dt_RHMC_f,
                       dt_RHMC_xy, True)
        self.R_accept = np.sum(self.A_chain[0, :] * 100) / float(self.Niter)
        print("Chain %d Acceptance rate: %.2f%%" % (0, self.R_accept))

    def RHMC_random_batched(self, q_model_0, Niter=1000, steps_min=10, steps_max=50, f_lim=0.,
                            f_lim_default=False, dt_RHMC_xy=1., dt_RHMC_f=0.1):
        """RHMC_random over many independent chains at once (q_model_0
        [Nchain, d], overwritten with the last states when it is float64); per
        iteration, i = 0 included, the global NumPy RNG draws randn(Nchain, d),
        and for i >= 1 randint(steps_min, steps_max, Nchain) and
        random(Nchain).  The R_accept stop applies per chain: a stopped chain's
        later rows stay zero and its draws are still consumed.  With one chain
        the chains equal RHMC_random's; only the position of the NumPy stream
        after an early stop differs (RHMC_random leaves the loop there, this
        method draws on to Niter).  Prints nothing."""
        self._set_f_lim(f_lim, f_lim_default)
        q0 = np.asarray(q_model_0, dtype=float)
        q0 = q0.reshape(1, -1) if q0.ndim == 1 else q0.reshape(q0.shape[0], -1)
        self.Nchain, self.d = q0.shape
        self.Nobjs = self.d // 3
        self.Niter = Niter
        self._run_hess(q0, Niter, steps_min, steps_max, dt_RHMC_f, dt_RHMC_xy, False)

    def _run_hess(self, q_tmp, Niter, steps_min, steps_max, dt_f, dt_xy, single):
        """The MH loop of samplers.py:978-1101 over the chains q_tmp [n, d],
        advanced in place.  Per iteration one trajectory launch, which also
        returns the derivative sets at its end state, and one launch for V
        there: the end state is the next iteration's start whether or not the
        proposal is accepted (q_initial aliases q_tmp, :982, :1031)."""
        ctx, P = self._context(), self._params()
        n, d = q_tmp.shape
        self.q_chain = np.zeros((n, Niter + 1, d))
        self.E_chain = np.zeros((n, Niter + 1, 1))
        self.dE_chain = np.zeros((n, Niter + 1, 1))
        self.A_chain = np.zeros((n, Niter, 1))
        _, dVdqq, _, V = ctx.hess_derivs(P, q_tmp, V=True)
        live = np.arange(n)             # chains the R_accept stop has not ended
        E_previous = np.zeros(n)
        for i in range(0, Niter + 1):
            z = self.p_sample() if single else np.random.randn(n, d)
            with np.errstate(all="ignore"):
                p_tmp = z.reshape(n, d) * np.sqrt(dVdqq)                      # :985-992
            E_initial = self._E_hess_batch(q_tmp, p_tmp, dVdqq, V)            # :998
            if i == 0:
                self.q_chain[:, 0, :] = q_tmp
                self.E_chain[:, 0, 0] = E_initial
                E_previous = E_initial
                continue
            steps = np.random.randint(low=steps_min, high=steps_max, size=n)  # :1013
            if live.size == 0:          # every chain stopped: the draws alone
                np.random.random(n)
                continue
            self.E_chain[live, i, 0] = E_initial[live]
            with np.errstate(invalid="ignore"):
                self.dE_chain[live, i, 0] = (E_initial - E_previous)[live]
            q_new, p_new, _, done, _, dVdqq_new, _ = ctx.hess_random(
                P, dt_f, dt_xy, q_tmp[live], p_tmp[live], steps[live], derivs=True)
            V_new = ctx.hess_derivs(P, q_new, V=True)[3]
            if single and done[0] < steps[0]:                                 # :1026
                print("Divergence encountered at (%d ,%d)" % (i, done[0]))
            E_final = self._E_hess_batch(q_new, p_new, dVdqq_new, V_new)      # :1076
            with np.errstate(invalid="ignore"):
                dE = E_final - E_initial[live]                                # :1081
            E_previous = E_initial
            lnu = np.log(np.random.random(n))[live]                           # :1083
            with np.errstate(invalid="ignore"):
                acc = (dE < 0) | (lnu < -dE)
            self.A_chain[live, i - 1, 0] = acc
            q_tmp[live] = q_new         # accepted or not: not restored (:1090-1091)
            dVdqq[live] = dVdqq_new
            V[live] = V_new
            self.q_chain[live, i, :] = q_new
            if (i % 100) == 0:                                                # :1098-1101
                R_accept = np.sum(self.A_chain[live, :i, 0] * 100, axis=1) / float(i)
                live = live[R_accept >= 50]
                if single and live.size == 0:
                    break

    def _run(self, q0, Niter, steps_min, steps_max):
        n, d = q0.shape
        self.q_chain = np.zeros((n, Niter + 1, d))
        self.E_chain = np.zeros((n, Niter + 1, 1))
        self.dE_chain = np.zeros((n, Niter + 1, 1))
        self.A_chain = np.zeros((n, Niter, 1))
        self.q_chain[:, 0, :] = q0
        p_initial = np.random.randn(n, d)
        self.E_chain[:, 0, 0] = self._E_batch(q0, p_initial)
        E_previous = self.E_chain[:, 0, 0].copy()
        q_tmp = q0.copy()
        for i in range(1, Niter + 1):
            q_initial = q_tmp
            p_tmp = np.random.randn(n, d)
            E_initial = self._E_batch(q_tmp, p_tmp)
            self.E_chain[:, i, 0] = E_initial
            self.dE_chain[:, i, 0] = E_initial - E_previous
            steps = np.random.randint(low=steps_min, high=steps_max, size=n)
            q_new, p_new = self._trajectories(q_tmp, p_tmp, steps)
            E_final = self._E_batch(q_new, p_new)
            with np.errstate(invalid="ignore"):
                dE = E_final - E_initial
            E_previous = E_initial
            lnu = np.log(np.random.random(n))
            with np.errstate(invalid="ignore"):
                acc = (dE < 0) | (lnu < -dE)
            self.A_chain[:, i - 1, 0] = acc
            q_tmp = np.where(acc[:, None], q_new, q_initial)
            self.q_chain[:, i, :] = q_tmp
