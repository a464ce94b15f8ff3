"""NumPy restatement of samplers.lightsource_gym.RHMC_random_diag, one chain at
a time, in the reference's expression order (jaekor91/HMC-stellar-toy-model
samplers.py; file:line below): mass_matrix / F / G / dlnDetdq / dpMpdq
(:574-664), V / dVdq / E / K (:1108-1173), the trajectory (:766-800) and the MH
loop around it (:719-823).  Test infrastructure only: the product runs the
trajectories in librhmc.so (rhmc_diag_random); the tests compare the two, and
test_diag_host.py pins this file to the fixture recorded from the reference
itself (tests/golden/make_goldens_diag.py).

Draws come from the global NumPy stream in the reference's order, or are
passed in (z, steps, lnu).
"""
import numpy as np

from peaks_ref import gauss_PSF


SCENES = ("k1", "k1fast", "k3", "wall", "traj")    # tests/golden/rhmc_diag.npz


def load_scene(z, name):
    """The arrays of one scene of the fixture archive z, without the prefix."""
    pre = name + "/"
    return {k[len(pre):]: z[k] for k in z.files if k.startswith(pre)}


def ref_of(s):
    """The DiagRef of a scene from load_scene()."""
    return DiagRef(s["D"].astype(float), float(s["B_count"]), float(s["fwhm_pix"]),
                   float(s["factor1"]))


def factor1_of(num_rows, num_cols, fwhm_pix):
    """compute_factors (:69-75) -> utils.factors' second value (utils.py:623-644)
    at the image centre."""
    x = num_rows / 2.
    y = num_cols / 2.
    lv = np.arange(0, num_rows)
    mv = np.arange(0, num_cols)
    mv, lv = np.meshgrid(lv, mv)
    var = (fwhm_pix / 2.354) ** 2
    PSF = gauss_PSF(num_rows, num_cols, x, y, FWHM=fwhm_pix)
    return np.sum(PSF * (x - lv - 0.5) ** 2) / float(var ** 2)


class DiagRef:
    """The potential, the diagonal metric and the sampler for one data image."""

    def __init__(self, D, B_count, fwhm_pix, factor1=None, scale_G=1.):
        self.D = np.asarray(D, dtype=float)
        self.num_rows, self.num_cols = self.D.shape
        self.B_count = B_count
        self.fwhm = fwhm_pix
        self.factor1 = factor1_of(self.num_rows, self.num_cols, fwhm_pix) \
            if factor1 is None else factor1
        lv = np.arange(0, self.num_rows)                          # :1124-1126
        mv = np.arange(0, self.num_cols)
        self.mv, self.lv = np.meshgrid(lv, mv)
        self.var = (fwhm_pix / 2.354) ** 2                        # :1127
        self.scale_G = scale_G      # the generator's sensitivity reruns

    def psf(self, x, y):
        return gauss_PSF(self.num_rows, self.num_cols, x, y, FWHM=self.fwhm)

    # ------------------------------------------------------------ potential
    def V(self, q):
        """:1137-1150."""
        with np.errstate(all="ignore"):
            Lambda = np.ones_like(self.D) * self.B_count
            for i in range(q.size // 3):
                f, x, y = q[3 * i:3 * i + 3]
                Lambda += f * self.psf(x, y)
            return -np.sum(self.D * np.log(Lambda) - Lambda)

    def dVdq(self, q):
        """:1108-1134."""
        with np.errstate(all="ignore"):
            grad = np.zeros(q.size)
            Lambda = np.ones_like(self.D) * self.B_count
            for i in range(q.size // 3):
                f, x, y = q[3 * i:3 * i + 3]
                Lambda += f * self.psf(x, y)
            rho = (self.D / Lambda) - 1.
            for i in range(q.size // 3):
                f, x, y = q[3 * i:3 * i + 3]
                PSF = self.psf(x, y)
                grad[3 * i] = -np.sum(rho * PSF)
                grad[3 * i + 1] = -np.sum(rho * (self.lv - x + 0.5) * PSF) * f / self.var
                grad[3 * i + 2] = -np.sum(rho * (self.mv - y + 0.5) * PSF) * f / self.var
            return grad * self.scale_G

    # --------------------------------------------------------------- metric
    def F(self, f):
        """:592-600 -> (F, dFdf)."""
        return f * self.factor1, self.factor1

    def G(self, f):
        """:614-625 -> (G, dGdf)."""
        with np.errstate(all="ignore"):
            return 1. / f, -1 / f ** 2

    def mass_matrix(self, q):
        """:574-590."""
        M = np.zeros_like(q)
        for i in range(q.shape[0] // 3):
            f = q[3 * i]
            M[3 * i] = self.G(f)[0]
            M[(3 * i) + 1:3 * (i + 1)] = self.F(f)[0]
        return M

    def dlnDetdq(self, q):
        """:636-649."""
        out = np.zeros_like(q)
        with np.errstate(all="ignore"):
            for i in range(q.shape[0] // 3):
                f = q[3 * i]
                G, dGdf = self.G(f)
                F, dFdf = self.F(f)
                out[3 * i] = 0.5 * (dGdf / G + 2 * dFdf / F)
        return out

    def dpMpdq(self, q, p):
        """:651-664."""
        out = np.zeros_like(q)
        with np.errstate(all="ignore"):
            for i in range(q.shape[0] // 3):
                f = q[3 * i]
                pf, px, py = p[3 * i:3 * (i + 1)]
                G, dGdf = self.G(f)
                F, dFdf = self.F(f)
                out[3 * i] = - 0.5 * (dGdf * pf ** 2 / G ** 2 + (px ** 2 + py ** 2) * dFdf / F ** 2)
        return out

    def force(self, q, p):
        """dVdq + dlnDetdq + dpMpdq, the sum of :766."""
        return self.dVdq(q) + self.dlnDetdq(q) + self.dpMpdq(q, p)

    # --------------------------------------------------------------- energy
    def K(self, p, M):
        """:1163-1173 with a mass matrix: a running product, then one log."""
        with np.errstate(all="ignore"):
            return (np.sum(p ** 2 / M) + np.log(np.abs(np.prod(M)))) / 2.

    def E(self, q, p, M, f_lim):
        """:1152-1161."""
        for l in range(q.size // 3):
            if q[3 * l] < f_lim:
                return np.inf
        with np.errstate(all="ignore"):
            return self.V(q) + self.K(p, M)

    # ----------------------------------------------------------- trajectory
    def traj(self, q, p, steps, dt, f_lim):
        """:766-800 from (q, p): (q, p, whether the last step flipped, q after
        every step [steps + 1, d]).  p is the input momentum when the last
        step flipped (the reference's stale momentum)."""
        q_tmp = np.array(q, dtype=float)
        p_tmp = np.array(p, dtype=float)
        d = q_tmp.size
        trace = np.zeros((steps + 1, d))
        trace[0] = q_tmp
        with np.errstate(all="ignore"):
            p_half = p_tmp - dt / 2. * self.force(q_tmp, p_tmp)              # :766
            iflip = np.zeros(d, dtype=bool)                                  # :767
            flip = False
            for i in range(steps):
                flip = False
                M = self.mass_matrix(q_tmp)                                  # :770
                q_tmp = q_tmp + dt * p_half / M                              # :771
                for l in range(d // 3):                                      # :775-778
                    if q_tmp[3 * l] < f_lim:
                        iflip[3 * l] = True
                        flip = True
                if flip:                                                     # :779-782
                    p_half_tmp = -p_half[iflip]
                    p_half = p_half - dt * self.force(q_tmp, p_tmp)
                    p_half[iflip] = p_half_tmp
                else:                                                        # :784
                    p_half = p_half - dt * self.force(q_tmp, p_tmp)
                trace[i + 1] = q_tmp
            if not flip:                                                     # :800
                p_tmp = p_half + dt * self.force(q_tmp, p_tmp) / 2.
        return q_tmp, p_tmp, flip, trace

    # -------------------------------------------------------------- MH loop
    def run(self, q0, Niter, dt, f_lim=0., steps_min=10, steps_max=50, z=None, steps=None,
            lnu=None, save_traj=False):
        """:719-823 for one chain from q0 [d].  Draws: z [Niter + 1, d] (row 0
        the draw of E_chain[0]), steps [Niter], lnu [Niter], or the global NumPy
        stream in the reference's order.  Returns a dict: q_chain [Niter + 1,
        d], E_chain, dE_chain [Niter + 1], A_chain [Niter], the draws used, the
        trajectories' end states q_end, p_end [Niter, d] and flipped_last
        [Niter], the MH test's dE [Niter]; with save_traj qs, Vs, Ts (lists,
        entry 0 the start, :734-737)."""
        q0 = np.array(q0, dtype=float).reshape(-1)
        d = q0.size
        drawn = z is None
        out = dict(q_chain=np.zeros((Niter + 1, d)), E_chain=np.zeros(Niter + 1),
                   dE_chain=np.zeros(Niter + 1), A_chain=np.zeros(Niter),
                   z=np.zeros((Niter + 1, d)), steps=np.zeros(Niter, np.int32),
                   lnu=np.zeros(Niter), q_end=np.zeros((Niter, d)), p_end=np.zeros((Niter, d)),
                   flipped_last=np.zeros(Niter, bool), dE=np.zeros(Niter))
        with np.errstate(all="ignore"):
            q_initial = q0
            M = self.mass_matrix(q_initial)                                  # :724
            out["z"][0] = np.random.randn(d) if drawn else z[0]
            p_initial = out["z"][0] * np.sqrt(M)                             # :725
            out["q_chain"][0] = q0
            out["E_chain"][0] = self.E(q_initial, p_initial, M, f_lim)       # :729
            E_previous = out["E_chain"][0]
            q_tmp = q_initial
            if save_traj:                                                    # :734-737
                out["qs"] = [np.array([q_initial])]
                out["Vs"] = [np.array([self.V(q_initial)])]
                out["Ts"] = [np.array([self.K(p_initial, M)])]
            for i in range(1, Niter + 1):
                q_initial = q_tmp
                M = self.mass_matrix(q_initial)                              # :745
                out["z"][i] = np.random.randn(d) if drawn else z[i]
                p_tmp = out["z"][i] * np.sqrt(M)                             # :746
                E_initial = self.E(q_tmp, p_tmp, M, f_lim)                   # :749
                out["E_chain"][i] = E_initial
                out["dE_chain"][i] = E_initial - E_previous
                n = (np.random.randint(low=steps_min, high=steps_max, size=1)[0]
                     if drawn else steps[i - 1])                             # :755
                out["steps"][i - 1] = n
                q_new, p_new, flip, trace = self.traj(q_tmp, p_tmp, int(n), dt, f_lim)
                if save_traj:                                                # :757-763, :787-790
                    out["qs"].append(trace)
                    out["Vs"].append(np.array([self.V(t) for t in trace]))
                    out["Ts"].append(np.array([self.K(p_tmp, self.mass_matrix(t))
                                               for t in trace]))
                out["q_end"][i - 1] = q_new
                out["p_end"][i - 1] = p_new
                out["flipped_last"][i - 1] = flip
                E_final = self.E(q_new, p_new, self.mass_matrix(q_new), f_lim)   # :803-804
                dE = E_final - E_initial                                     # :807
                out["dE"][i - 1] = dE
                E_previous = E_initial
                out["lnu"][i - 1] = (np.log(np.random.random(1))[0] if drawn
                                     else lnu[i - 1])                        # :809
                if (dE < 0) or (out["lnu"][i - 1] < -dE):                    # :810-815
                    out["A_chain"][i - 1] = 1
                    q_tmp = q_new
                else:
                    q_tmp = q_initial
                out["q_chain"][i] = q_tmp
        return out
