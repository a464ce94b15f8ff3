"""NumPy restatement of samplers.lightsource_gym.RHMC_random, one chain at a
time, in the reference's expression order (jaekor91/HMC-stellar-toy-model
samplers.py; file:line below): RHMC_efficient_computation (:828-927), the
trajectory (:1016-1067) and the MH loop around it (:974-1103).  Test
infrastructure only: the product runs the derivative sets and the trajectories
in librhmc.so (rhmc_hess_derivs, rhmc_hess_random); the tests compare the two,
and test_hess_host.py pins this file to the fixture recorded from the reference
itself (tests/golden/make_goldens_hess.py).

Draws come from the global NumPy stream in the reference's order, or are
passed in (z, steps, lnu).  The derivative sums depend on q alone, so they are
computed once per state and reused by the calls that differ only in p.
"""
import numpy as np

from peaks_ref import gauss_PSF

SCENES = ("k1", "k1slow", "k3", "wall", "stop")     # tests/golden/rhmc_hess.npz
FUNCTIONS = ("fn1", "fn3", "fn10")                  # its RHMC_efficient_computation records

STATUS_NONFINITE, STATUS_REFLECT_F, STATUS_REFLECT_XY = 1, 8, 16   # include/rhmc.h


def load_scene(z, name):
    """The arrays of one scene of the fixture archive z, without the prefix."""
    pre = name + "/"
    return {k[len(pre):]: z[k] for k in z.files if k.startswith(pre)}


def ref_of(s, scale_G=1.):
    """The HessRef of a scene from load_scene()."""
    return HessRef(s["D"].astype(float), float(s["B_count"]), float(s["fwhm_pix"]),
                   scale_G=scale_G)


class HessRef:
    """The potential, its first three diagonal derivatives and the sampler for
    one data image."""

    def __init__(self, D, B_count, fwhm_pix, scale_G=1.):
        self.D = np.asarray(D, dtype=float)
        self.num_rows, self.num_cols = self.D.shape
        self.B_count = B_count
        self.fwhm = fwhm_pix
        lv = np.arange(0, self.num_rows) + 0.5                        # :855-857
        mv = np.arange(0, self.num_cols) + 0.5
        self.mv, self.lv = np.meshgrid(lv, mv)
        self.var = (fwhm_pix / 2.354) ** 2                            # :858
        self.scale_G = scale_G      # the generator's sensitivity reruns

    def psf(self, x, y):
        return gauss_PSF(self.num_rows, self.num_cols, x, y, FWHM=self.fwhm)

    def Lambda(self, q):
        """:845-848."""
        Lambda = np.ones_like(self.D) * self.B_count
        for k in range(q.size // 3):
            f, x, y = q[3 * k:3 * k + 3]
            Lambda += f * self.psf(x, y)
        return Lambda

    def V(self, q):
        """:912."""
        with np.errstate(all="ignore"):
            Lambda = self.Lambda(q)
            return -np.sum(self.D * np.log(Lambda) - Lambda)

    def derivs(self, q, scales=False):
        """:840-903 -> (dVdq, dVdqq, dVdqqq) [d], each times scale_G; with scales
        also each derivative's scale, the sum over pixels and terms of |term|."""
        q = np.asarray(q, dtype=float)
        d = q.size
        dVdq, dVdqq, dVdqqq = np.zeros(d), np.zeros(d), np.zeros(d)
        s1, s2, s3 = np.zeros(d), np.zeros(d), np.zeros(d)
        var, lv, mv = self.var, self.lv, self.mv
        A = np.abs
        with np.errstate(all="ignore"):
            Lambda = self.Lambda(q)
            rho0 = self.D / Lambda                                    # :851-854
            rho1 = 1 - rho0
            rho2 = rho0 / Lambda
            rho3 = rho2 / Lambda
            for k in range(d // 3):
                f, x, y = q[3 * k:3 * k + 3]
                PSF = self.psf(x, y)                                  # :865-877
                PSF_sq = PSF ** 2
                PSF_cube = PSF_sq * PSF
                dPSFdx = PSF * (lv - x) / var
                dPSFdx_sq = dPSFdx ** 2
                dPSFdxx = (dPSFdx * (lv - x) - PSF) / var
                dPSFdxxx = (dPSFdxx * (lv - x) - 2 * dPSFdx) / var
                dPSFdy = PSF * (mv - y) / var
                dPSFdy_sq = dPSFdy ** 2
                dPSFdyy = (dPSFdy * (mv - y) - PSF) / var
                dPSFdyyy = (dPSFdyy * (mv - y) - 2 * dPSFdy) / var
                dVdf = np.sum(rho1 * PSF)                             # :881-893
                dVdff = np.sum(rho2 * PSF_sq)
                dVdfff = -2 * np.sum(rho3 * PSF_cube)
                dVdx = f * np.sum(rho1 * dPSFdx)
                dVdxx = f ** 2 * np.sum(rho2 * dPSFdx_sq) + f * np.sum(rho1 * dPSFdxx)
                dVdxxx = - f ** 3 * np.sum(rho3 * dPSFdx_sq * dPSFdx) \
                    + 3 * f ** 2 * np.sum(rho2 * dPSFdx * dPSFdxx) \
                    + f * np.sum(rho1 * dPSFdxxx)
                dVdy = f * np.sum(rho1 * dPSFdy)
                dVdyy = f ** 2 * np.sum(rho2 * dPSFdy_sq) + f * np.sum(rho1 * dPSFdyy)
                dVdyyy = - f ** 3 * np.sum(rho3 * dPSFdy_sq * dPSFdy) \
                    + 3 * f ** 2 * np.sum(rho2 * dPSFdy * dPSFdyy) \
                    + f * np.sum(rho1 * dPSFdyyy)
                dVdq[3 * k:3 * (k + 1)] = np.array([dVdf, dVdx, dVdy])
                dVdqq[3 * k:3 * (k + 1)] = np.array([dVdff, dVdxx, dVdyy])
                dVdqqq[3 * k:3 * (k + 1)] = np.array([dVdfff, dVdxxx, dVdyyy])
                if scales:
                    af = abs(f)
                    s1[3 * k:3 * (k + 1)] = [
                        np.sum(A(rho1 * PSF)), af * np.sum(A(rho1 * dPSFdx)),
                        af * np.sum(A(rho1 * dPSFdy))]
                    s2[3 * k:3 * (k + 1)] = [
                        np.sum(A(rho2 * PSF_sq)),
                        af ** 2 * np.sum(A(rho2 * dPSFdx_sq)) + af * np.sum(A(rho1 * dPSFdxx)),
                        af ** 2 * np.sum(A(rho2 * dPSFdy_sq)) + af * np.sum(A(rho1 * dPSFdyy))]
                    s3[3 * k:3 * (k + 1)] = [
                        2 * np.sum(A(rho3 * PSF_cube)),
                        af ** 3 * np.sum(A(rho3 * dPSFdx_sq * dPSFdx))
                        + 3 * af ** 2 * np.sum(A(rho2 * dPSFdx * dPSFdxx))
                        + af * np.sum(A(rho1 * dPSFdxxx)),
                        af ** 3 * np.sum(A(rho3 * dPSFdy_sq * dPSFdy))
                        + 3 * af ** 2 * np.sum(A(rho2 * dPSFdy * dPSFdyy))
                        + af * np.sum(A(rho1 * dPSFdyyy))]
        out = (dVdq * self.scale_G, dVdqq * self.scale_G, dVdqqq * self.scale_G)
        return out + ((s1, s2, s3),) if scales else out

    def compute(self, q, p, f_lim, dVdqq_only=False, d=None):
        """RHMC_efficient_computation (:828-927) with the reference's three
        return shapes: dVdqq [d]; (inf, inf, inf) below the wall; (dqdt, dpdt,
        E).  d: derivs(q) from an earlier call at the same q."""
        if not dVdqq_only:
            for k in range(q.size // 3):                              # :832-837
                if q[3 * k] < f_lim:
                    return np.inf, np.inf, np.inf
        dVdq, dVdqq, dVdqqq = self.derivs(q) if d is None else d
        if dVdqq_only:
            return dVdqq
        with np.errstate(all="ignore"):
            dqdt = p / dVdqq                                          # :909-913
            dpdt = -dVdqqq * ((1. / dVdqq) - dqdt ** 2) / 2. - dVdq
            K = np.sum((p ** 2) / dVdqq) / 2. + np.log(np.prod(dVdqq)) / 2.
            E = K + self.V(q)
        return dqdt, dpdt, E

    # ----------------------------------------------------------- trajectory
    def traj(self, q, p, steps, dt, f_lim):
        """:1016-1076 from (q, p), q advanced IN PLACE like the reference's
        q_tmp: a dict with q (the same array), p (p_half as it is left),
        steps_done, status (RHMC_STATUS_* bits), E_final (:1076), d (the
        derivative sets at the end q) and diverged_at (the z of :1026 or None)."""
        d = q.size
        n_obj = d // 3
        with np.errstate(all="ignore"):
            dq = self.derivs(q)
            dqdt, dpdt, E = self.compute(q, p, f_lim, d=dq)
            p_half = p + dt * dpdt / 2.                               # :1016
            iflip = np.zeros(d, dtype=bool)
            iflip_x = np.zeros(d, dtype=bool)
            iflip_y = np.zeros(d, dtype=bool)
            done, diverged_at = 0, None
            for z in range(steps):
                dqdt, dpdt, E = self.compute(q, p_half, f_lim, d=dq)  # :1024
                if E == np.inf:
                    diverged_at = z
                    break
                flip = flip_x = flip_y = False
                q += dt * dqdt                                        # :1031
                for l in range(n_obj):                                # :1034-1043
                    if q[3 * l] < f_lim:
                        iflip[3 * l] = True
                        flip = True
                    if (q[3 * l + 1] < 0) or (q[3 * l + 1] < self.num_rows):
                        iflip_x[3 * l + 1] = True
                        flip_x = True
                    if (q[3 * l + 2] < 0) or (q[3 * l + 2] < self.num_rows):
                        iflip_y[3 * l + 2] = True
                        flip_y = True
                dt_tmp = dt / 2. if z == steps - 1 else dt            # :1046-1049
                dq = self.derivs(q)
                dqdt, dpdt, E = self.compute(q, p_half, f_lim, d=dq)  # :1054
                p_half_tmp = -p_half                                  # :1057-1067
                p_half = p_half + dt_tmp * dpdt
                if flip:
                    p_half[iflip] = p_half_tmp[iflip]
                if flip_x:
                    p_half[iflip_x] = p_half_tmp[iflip_x]
                if flip_y:
                    p_half[iflip_y] = p_half_tmp[iflip_y]
                done += 1
            E_final = self.compute(q, p_half, f_lim, d=dq)[2]         # :1076
        status = (STATUS_REFLECT_F if iflip.any() else 0) \
            | (STATUS_REFLECT_XY if (iflip_x.any() or iflip_y.any()) else 0) \
            | (0 if (np.isfinite(q).all() and np.isfinite(p_half).all()) else STATUS_NONFINITE)
        return dict(q=q, p=p_half, steps_done=done, status=status, E_final=E_final, d=dq,
                    diverged_at=diverged_at)

    # -------------------------------------------------------------- MH loop
    def run(self, q0, Niter, dt_f, dt_xy, f_lim=0., steps_min=10, steps_max=50, z=None,
            steps=None, lnu=None):
        """:974-1103 for one chain from q0 [d], which is advanced IN PLACE like
        the reference's q_model_0 (a rejected proposal is not restored: q_initial
        aliases q_tmp, :982, :1031).  Draws: z [Niter + 1, d] (row 0 the draw of
        E_chain[0]), steps [Niter], lnu [Niter], or the global NumPy stream in
        the reference's order.  Returns a dict: q_chain [Niter + 1, d], E_chain,
        dE_chain [Niter + 1], A_chain [Niter], the draws used, per iteration the
        trajectory's end state q_end, p_end [Niter, d], steps_done, status, the
        MH test's dE, n_run (iterations run before the R_accept stop of
        :1098-1101, else Niter) and lines (what the reference prints)."""
        q_tmp = q0.reshape(-1)
        assert q_tmp.dtype == np.float64 and np.shares_memory(q_tmp, q0)
        d = q_tmp.size
        dt = np.asarray([dt_f, dt_xy, dt_xy] * (d // 3))              # :952
        drawn = z is None
        out = dict(q_chain=np.zeros((Niter + 1, d)), E_chain=np.zeros(Niter + 1),
                   dE_chain=np.zeros(Niter + 1), A_chain=np.zeros(Niter),
                   z=np.zeros((Niter + 1, d)), steps=np.zeros(Niter, np.int32),
                   lnu=np.zeros(Niter), q_end=np.zeros((Niter, d)), p_end=np.zeros((Niter, d)),
                   steps_done=np.zeros(Niter, np.int32), status=np.zeros(Niter, np.int32),
                   dE=np.zeros(Niter), n_run=Niter, lines=[])
        with np.errstate(all="ignore"):
            E_previous = 0.
            for i in range(0, Niter + 1):
                dq = self.derivs(q_tmp)
                out["z"][i] = np.random.randn(d) if drawn else z[i]
                p_tmp = out["z"][i] * np.sqrt(dq[1])                  # :985-992
                E = self.compute(q_tmp, p_tmp, f_lim, d=dq)[2]        # :998
                if i == 0:
                    out["q_chain"][0] = q_tmp
                    out["E_chain"][0] = E
                    E_previous = E
                    continue
                E_initial = E
                out["E_chain"][i] = E_initial
                out["dE_chain"][i] = E_initial - E_previous
                n = (np.random.randint(low=steps_min, high=steps_max, size=1)[0]
                     if drawn else steps[i - 1])                      # :1013
                out["steps"][i - 1] = n
                t = self.traj(q_tmp, p_tmp, int(n), dt, f_lim)
                if t["diverged_at"] is not None:
                    out["lines"].append("Divergence encountered at (%d ,%d)"
                                        % (i, t["diverged_at"]))
                out["q_end"][i - 1] = q_tmp
                out["p_end"][i - 1] = t["p"]
                out["steps_done"][i - 1] = t["steps_done"]
                out["status"][i - 1] = t["status"]
                dE = t["E_final"] - E_initial                         # :1081
                out["dE"][i - 1] = dE
                E_previous = E_initial
                out["lnu"][i - 1] = (np.log(np.random.random(1))[0] if drawn
                                     else lnu[i - 1])                 # :1083
                if (dE < 0) or (out["lnu"][i - 1] < -dE):             # :1084-1091
                    out["A_chain"][i - 1] = 1
                out["q_chain"][i] = q_tmp       # accepted or not: q_initial IS q_tmp
                if (i % 100) == 0:                                    # :1098-1101
                    if np.sum(out["A_chain"][:i] * 100) / float(i) < 50:
                        out["n_run"] = i
                        break
        out["lines"].append("Chain %d Acceptance rate: %.2f%%"
                            % (0, np.sum(out["A_chain"] * 100) / float(Niter)))
        return out
