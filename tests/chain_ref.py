"""CPU replay of rhmc_chain (include/rhmc.h), one chain at a time on given
draws, built on the oracle's HMC_random pieces (oracle.rhmc_ref.RefModel.ls_E /
hmc_random_traj) and the RHMC_random_diag restatement (rhmc_diag_ref.DiagRef).
Test infrastructure only: tests/test_chain_host.py uses it as the stand-in for
capi.Context.chain, tests/test_gpu_chain.py as the reference of the device
engine and for the margin of every accept decision.
"""
import numpy as np

from oracle import rhmc_ref as R
import rhmc_diag_ref


def unit_model(D, B_count, fwhm_pix, f_lim=0.):
    """The oracle model of lightsource_gym on image D (no prior, unit metric)."""
    n = D.shape[0]
    par = dict(rows=n, cols=n, B_count=float(B_count), fwhm_pix=float(fwhm_pix), use_prior=0,
               use_Vc=0, alpha=2., beta=1., Vc_r_pow=1., dt=1., f_lim=float(f_lim), f_low=1.,
               g_xx=1., g_ff=1., g_ff2=1., g0=1., g1=1., g2=1., fmin=-1., fmax=-1.)
    return R.RefModel(np.asarray(D, dtype=float), par)


class ChainRef:
    """E and the trajectory of one metric on one image."""

    def __init__(self, D, B_count, fwhm_pix, metric, f_lim, dt=None, dt_global=None,
                 factor1=None):
        self.metric, self.f_lim = metric, float(f_lim)
        if metric == "unit":
            self.m = unit_model(D, B_count, fwhm_pix, f_lim)
            self.dt = np.asarray(dt, dtype=float)
        else:
            self.m = rhmc_diag_ref.DiagRef(D, B_count, fwhm_pix, factor1)
            self.dt = float(dt_global)

    def momentum(self, q, z):
        if self.metric == "unit":
            return np.array(z, dtype=float)
        with np.errstate(all="ignore"):
            return z * np.sqrt(self.m.mass_matrix(q))

    def E(self, q, p):
        with np.errstate(all="ignore"):
            if self.metric == "unit":
                return self.m.ls_E(q, p, self.f_lim)
            return self.m.E(q, p, self.m.mass_matrix(q), self.f_lim)

    def traj(self, q, p, steps):
        with np.errstate(all="ignore"):
            if self.metric == "unit":
                return self.m.hmc_random_traj(q.copy(), p.copy(), self.dt, int(steps),
                                              self.f_lim)[:3]
            return self.m.traj(q, p, int(steps), self.dt, self.f_lim)[:3]

    def run(self, q0, z, steps, lnu):
        """rhmc_chain on the chains q0 [n, d] with the draws z [ni + 1, n, d],
        steps [ni, n], lnu [ni, n]: the record of capi.Context.chain
        (iteration-major) plus E_final and dE of every decision [ni, n] and
        flipped [ni, n] (the trajectory ended on a flipped step)."""
        q0 = np.array(q0, dtype=float)
        n, d = q0.shape
        ni = steps.shape[0]
        out = dict(q_chain=np.zeros((ni + 1, n, d)), E_chain=np.zeros((ni + 1, n)),
                   dE_chain=np.zeros((ni + 1, n)), accept=np.zeros((ni, n), np.int32),
                   z=np.array(z, dtype=float), steps=np.array(steps, np.int32),
                   lnu=np.array(lnu, dtype=float), E_final=np.zeros((ni, n)),
                   dE=np.zeros((ni, n)), flipped=np.zeros((ni, n), bool), q=q0.copy())
        with np.errstate(all="ignore"):
            for c in range(n):
                q = q0[c].copy()
                out["q_chain"][0, c] = q
                E_prev = out["E_chain"][0, c] = self.E(q, self.momentum(q, z[0, c]))
                for i in range(1, ni + 1):
                    p = self.momentum(q, z[i, c])
                    Ei = out["E_chain"][i, c] = self.E(q, p)
                    out["dE_chain"][i, c] = Ei - E_prev
                    E_prev = Ei
                    qn, pn, flip = self.traj(q, p, steps[i - 1, c])
                    Ef = out["E_final"][i - 1, c] = self.E(qn, pn)
                    dE = out["dE"][i - 1, c] = Ef - Ei
                    out["flipped"][i - 1, c] = flip
                    if (dE < 0) or (lnu[i - 1, c] < -dE):
                        out["accept"][i - 1, c] = 1
                        q = np.array(qn, dtype=float)
                    out["q_chain"][i, c] = q
                out["q"][c] = q
        return out


def margins(run):
    """|lnu + dE| / (|E_initial| + |E_final|) of every decision with a finite
    dE (the others are decided by inf / NaN, which no rounding moves)."""
    dE, lnu = run["dE"], run["lnu"]
    Ei, Ef = run["E_chain"][1:], run["E_final"]
    fin = np.isfinite(dE)
    return np.abs(lnu + dE)[fin] / (np.abs(Ei) + np.abs(Ef))[fin]


def draw_numpy(n, d, Niter, steps_min, steps_max):
    """The host loop's draws from the global NumPy stream, in its order."""
    z = np.empty((Niter + 1, n, d))
    steps = np.empty((Niter, n), np.int32)
    lnu = np.empty((Niter, n))
    z[0] = np.random.randn(n, d)
    for i in range(Niter):
        z[i + 1] = np.random.randn(n, d)
        steps[i] = np.random.randint(low=steps_min, high=steps_max, size=n)
        lnu[i] = np.log(np.random.random(n))
    return z, steps, lnu
