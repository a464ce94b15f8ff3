"""NumPy restatement of HMC_find_best_dt's step-size search, in the reference's
expression order (jaekor91/HMC-stellar-toy-model samplers.py; file:line below):
the trial (:332-371, identical at :399-438) with both gradient forms, and the
coarse / fine search around it (:306-456).  Test infrastructure only: the
product runs the trials in librhmc.so (rhmc_dt_trials); the tests compare the
two, and test_dt_host.py pins this file to the fixture recorded from the
reference itself (tests/golden/make_goldens_dt.py).

Draws come from the global NumPy stream in the reference's order, or are
passed in (z, steps, lnu).
"""
import numpy as np

from peaks_ref import gauss_PSF

FLUX, XY = 0, 1            # phase k (:317)
COARSE, FINE = 0, 1        # stage
COARSE_CAP = 64            # trials of one coarse loop before the search gives up


class DtRef:
    """V_single / dVdq_single / E_single (:77-127) for one data image."""

    def __init__(self, D, fwhm_pix, scale_G=1., scale_V=1.):
        self.D = np.asarray(D, dtype=float)
        self.num_rows, self.num_cols = self.D.shape
        self.fwhm = fwhm_pix
        lv = np.arange(0, self.num_rows)                      # :95-97
        mv = np.arange(0, self.num_cols)
        self.mv, self.lv = np.meshgrid(lv, mv)
        self.var = (fwhm_pix / 2.354) ** 2                    # :98
        self.scale_G = scale_G      # the generator's robustness reruns
        self.scale_V = scale_V
        self.E_log = None           # a list: every E_single value, in call order

    def psf(self, x, y):
        return gauss_PSF(self.num_rows, self.num_cols, x, y, FWHM=self.fwhm)

    def V(self, q, M):
        """V_single, :121-127."""
        f0, x0, y0 = q
        with np.errstate(all="ignore"):
            Lambda = M + f0 * self.psf(x0, y0)
            return -np.sum(self.D * np.log(Lambda) - Lambda) * self.scale_V

    def E(self, q, p, M):
        """E_single, :114-118."""
        with np.errstate(all="ignore"):
            e = self.V(q, M) + np.dot(p, p) / 2.
        if self.E_log is not None:
            self.E_log.append(float(e))
        return e

    def G(self, q, M, grad="reference"):
        """dVdq_single: f_only=True (:102-104), what the search's call gives (a
        scalar, broadcast over the coordinates by `dt * G`), or return_all
        (:93-101) as an array."""
        f, x, y = q
        with np.errstate(all="ignore"):
            Lambda = M + f * self.psf(x, y)                   # :85
            rho = (self.D / Lambda) - 1.                      # :88
            PSF = self.psf(x, y)                              # :91
            grad_f = -np.sum(rho * PSF)                       # :94 / :103
            if grad == "reference":
                return grad_f * self.scale_G
            grad_x = -np.sum(rho * (self.lv - x + 0.5) * PSF) * f / self.var   # :99
            grad_y = -np.sum(rho * (self.mv - y + 0.5) * PSF) * f / self.var   # :100
            return np.array([grad_f, grad_x, grad_y]) * self.scale_G

    def trial(self, q0, dt, M, n_iter, flux_only, grad="reference", z=None, steps=None,
              lnu=None, steps_min=10, steps_max=50):
        """:332-371.  Returns a dict: n_accept and per iteration z, steps, lnu
        (the draws used), dE, accept, q (after the iteration)."""
        dt = np.asarray(dt, dtype=float)
        q_tmp = np.array(q0, dtype=float)                     # :335
        out = dict(z=np.zeros((n_iter, 3)), steps=np.zeros(n_iter, np.int32),
                   lnu=np.zeros(n_iter), dE=np.zeros(n_iter), accept=np.zeros(n_iter, np.int32),
                   q=np.zeros((n_iter, 3)))
        n_accept = 0
        with np.errstate(all="ignore"):
            for i in range(n_iter):                           # :338
                q_initial = q_tmp
                p_tmp = np.random.randn(3) if z is None else np.array(z[i], dtype=float)   # :343
                out["z"][i] = p_tmp
                if flux_only:
                    p_tmp[1:] = 0                             # :344-345
                E_initial = self.E(q_tmp, p_tmp, M)           # :348
                if steps is None:
                    steps_sample = np.random.randint(low=steps_min, high=steps_max, size=1)[0]
                else:
                    steps_sample = int(steps[i])
                p_half = p_tmp - dt * self.G(q_tmp, M, grad) / 2.       # :352
                for _ in range(steps_sample):                 # :354-356
                    q_tmp = q_tmp + dt * p_half
                    p_half = p_half - dt * self.G(q_tmp, M, grad)
                p_tmp = p_half + dt * self.G(q_tmp, M, grad) / 2.       # :357
                E_final = self.E(q_tmp, p_tmp, M)             # :360
                dE = E_final - E_initial                      # :363
                u_ln = np.log(np.random.random(1))[0] if lnu is None else float(lnu[i])   # :365
                accept = bool((dE < 0) or (u_ln < -dE))       # :366
                if accept:
                    n_accept += 1
                else:
                    q_tmp = q_initial
                out["steps"][i] = steps_sample
                out["lnu"][i] = u_ln
                out["dE"][i] = dE
                out["accept"][i] = accept
                out["q"][i] = q_tmp
        out["n_accept"] = n_accept
        return out


def search(ref, q_model_0, gen_mock, steps_min=10, steps_max=50, Niter_per_trial=10, Ntrial=10,
           dt_f_coeff=1., dt_xy_coeff=10., A_target_f=0.9, A_target_xy=0.5, grad="reference",
           run_trial=None, log=None):
    """:306-456.  gen_mock() draws the Poisson realisation of q_model_0's model
    (gen_mock_data(q_model_0, return_data=True), :314).  run_trial(l, k, stage,
    q0, dt, M) -> number accepted, default ref.trial with draws from the
    global stream.  log: a list that receives one dict per trial (star, phase,
    stage, dt, A_rate, the background M and ref.trial's record).  Returns the step vector
    [3 Nobjs]."""
    q_model_0 = np.asarray(q_model_0, dtype=float).reshape(-1, 3)
    Nobjs = q_model_0.shape[0]
    dt_out = np.zeros(3 * Nobjs)

    def one(l, k, stage, q0, dt, M):
        if run_trial is not None:
            return run_trial(l, k, stage, q0, dt, M)
        r = ref.trial(q0, dt, M, Niter_per_trial, k == FLUX, grad, steps_min=steps_min,
                      steps_max=steps_max)
        if log is not None:
            log.append(dict(r, star=l, phase=k, stage=stage, dt=np.array(dt), M=M,
                            A_rate=r["n_accept"] / float(Niter_per_trial)))
        return r["n_accept"]

    for l in range(Nobjs):
        f0, x0, y0 = q_model_0[l]
        dt_xy = dt_xy_coeff / f0                              # :310-311
        dt_f = dt_f_coeff * f0
        model_data = gen_mock()                               # :314
        model_data -= f0 * ref.psf(x0, y0)                    # :315
        q0 = np.array([f0, x0, y0])
        for k in range(2):                                    # :317
            if k == 0:
                dt = np.array([dt_f, 0, 0])
                A_target = A_target_f
            else:
                dt = np.array([dt_f, dt_xy, dt_xy])
                A_target = A_target_xy
            n_coarse = 0
            while True:                                       # :330
                if n_coarse == COARSE_CAP:
                    raise RuntimeError("HMC_find_best_dt: star %d did not reach the target "
                                       "acceptance in %d coarse trials" % (l, COARSE_CAP))
                n_coarse += 1
                A_rate = one(l, k, COARSE, q0, dt, model_data) / float(Niter_per_trial)   # :371
                if A_rate < A_target:                         # :374-378
                    if k == 0:
                        dt /= 10.
                    else:
                        dt[1:] = dt[1:] / 10.
                else:
                    break
            counter = 0                                       # :383-387
            dt_left = dt
            dt_right = 10. * dt
            if k == 1:
                dt_right[0] = dt_f
            while counter < Ntrial:                           # :390
                counter += 1
                dt = (dt_left + dt_right) / 2.                # :394
                if k == 1:
                    dt[0] = dt_f
                A_rate = one(l, k, FINE, q0, dt, model_data) / float(Niter_per_trial)     # :438
                if np.abs(A_rate - A_target) < 1e-2:          # :441-446
                    break
                elif A_rate > A_target:
                    dt_left = dt
                else:
                    dt_right = dt
            if k == 0:                                        # :450-453
                dt_f = dt[0]
            else:
                dt_xy = dt[1] * 10
        dt_out[3 * l:3 * l + 3] = np.array([dt_f, dt_xy, dt_xy])       # :456
    return dt_out


# ---- the fixture tests/golden/find_best_dt.npz --------------------------------

SCENES = ("A", "B", "C", "D", "E", "F")
COMPARED_DE = 50.          # an iteration is compared in value when |dE| <= this (finite)


def compared(dE):
    with np.errstate(invalid="ignore"):
        return np.isfinite(dE) & (np.abs(dE) <= COMPARED_DE)


def load_scene(z, name, grad="reference"):
    """One recorded search of a scene as arrays over its trials: the data
    image D, the backgrounds M [Nobjs] rebuilt from the stored realisations
    (M = realisation - f0 PSF, samplers.py:314-315), and per trial q0, dt,
    flux_only, bg_index (= star) and the recorded draws and results."""
    from rhmc_amd.photometry import gauss_PSF as psf
    pre = name + "/" + ("full/" if grad == "full" else "")
    side = int(z[name + "/side"])
    fwhm = float(z[name + "/fwhm_pix"])
    q_model_0 = z[name + "/q_model_0"]
    reals = z[pre + "realisations"].astype(float)
    M = np.array([reals[l] - q_model_0[l, 0] * psf(side, side, q_model_0[l, 1], q_model_0[l, 2],
                                                   FWHM=fwhm) for l in range(len(q_model_0))])
    star = z[pre + "star"]
    s = dict(name=name, grad=grad, side=side, fwhm=fwhm, B_count=float(z[name + "/B_count"]),
             D=z[name + "/D"].astype(float), q_model_0=q_model_0, M=M, star=star,
             seed=int(z[name + "/seed"]), search_seed=int(z[pre + "search_seed"]),
             n_iter=int(z[name + "/n_iter"]), q0=q_model_0[star], dt=z[pre + "trial_dt"],
             flux_only=(z[pre + "phase"] == FLUX).astype(np.int32), dt_final=z[pre + "dt"],
             next_random=float(z[pre + "next_random"]))
    for k in ("phase", "stage", "A_rate", "z", "steps", "lnu", "dE", "accept", "q",
              "realisations"):
        s[k] = z[pre + k]
    return s
