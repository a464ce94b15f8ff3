"""NumPy restatement of find_peaks' seed descent, in the reference's expression
order (jaekor91/HMC-stellar-toy-model samplers.py; file:line below).  Test
infrastructure only: the product runs the descent in librhmc.so
(rhmc_find_peaks); the tests compare the two, and test_peaks_host.py pins this
file to the fixture recorded from the reference itself.
"""
import math

import numpy as np

FAINT, CONVERGED, CAP = "faint", "converged", "cap"


def gauss_PSF(num_rows, num_cols, x, y, FWHM):
    """utils.py:475-486."""
    sigma = FWHM / 2.354
    xv = np.arange(0.5, num_rows)
    yv = np.arange(0.5, num_cols)
    yv, xv = np.meshgrid(xv, yv)
    return np.exp(-(np.square(xv - x) + np.square(yv - y)) / (2 * sigma ** 2)) \
        / (np.pi * 2 * sigma ** 2)


class PeaksRef:
    """The one-star potential and gradient against a pure-background model
    (samplers.py:187-188) for one image."""

    def __init__(self, D, B_count, fwhm_pix):
        self.D = np.asarray(D, dtype=float)
        self.num_rows, self.num_cols = self.D.shape
        self.fwhm = fwhm_pix
        self.model = np.ones((self.num_rows, self.num_cols), dtype=float) * B_count   # :188
        lv = np.arange(0, self.num_rows)                                             # :95-97
        mv = np.arange(0, self.num_cols)
        self.mv, self.lv = np.meshgrid(lv, mv)
        self.var = (fwhm_pix / 2.354) ** 2                                           # :98

    def V(self, f, x, y, fsum=False):
        """V_single, samplers.py:121-127 (fsum: the same terms summed exactly)."""
        Lambda = self.model + f * gauss_PSF(self.num_rows, self.num_cols, x, y, FWHM=self.fwhm)
        with np.errstate(invalid="ignore", divide="ignore"):
            t = self.D * np.log(Lambda) - Lambda
        return -math.fsum(t.ravel()) if fsum else -np.sum(t)

    def dVdq(self, f, x, y):
        """dVdq_single(return_all=True), samplers.py:84-101."""
        PSF = gauss_PSF(self.num_rows, self.num_cols, x, y, FWHM=self.fwhm)
        Lambda = self.model + f * PSF
        with np.errstate(invalid="ignore", divide="ignore"):
            rho = (self.D / Lambda) - 1.
        grad_f = -np.sum(rho * PSF)
        grad_x = -np.sum(rho * (self.lv - x + 0.5) * PSF) * f / self.var
        grad_y = -np.sum(rho * (self.mv - y + 0.5) * PSF) * f / self.var
        return grad_f, grad_x, grad_y

    def descend(self, q, f_lim, n_step=1000, dt_f_coeff=1e-1, dt_xy_coeff=1e-1, rel_tol=1e-9,
                force_steps=None, trace=None):
        """samplers.py:192-221 for one seed q = (f, x, y).  Returns
        (f, x, y, steps, reason, V_last): steps = gradient evaluations, V_last
        = the last V evaluated.  force_steps: take exactly that many steps
        with both tests off (reason None).  trace: a list that receives
        (ratio, f) per step (ratio None on the faint step)."""
        f, x, y = (float(v) for v in q)
        V_previous = self.V(f, x, y)                                                 # :195
        V_last = V_previous
        n = n_step if force_steps is None else force_steps
        with np.errstate(all="ignore"):
            for i in range(n):                                                       # :197
                grad_f, grad_x, grad_y = self.dVdq(f, x, y)                          # :198
                dt_f = f * dt_f_coeff                                                # :201
                dt_xy = dt_xy_coeff / f                                              # :202
                f -= grad_f * dt_f                                                   # :205-207
                x -= grad_x * dt_xy
                y -= grad_y * dt_xy
                if force_steps is None and f < f_lim:                                # :209
                    if trace is not None:
                        trace.append((None, f))
                    return f, x, y, i + 1, FAINT, V_last
                V_current = self.V(f, x, y)                                          # :213
                V_last = V_current
                ratio = np.abs((V_current - V_previous) / V_previous)                # :215
                if trace is not None:
                    trace.append((ratio, f))
                if force_steps is None and ratio < rel_tol:
                    return f, x, y, i + 1, CONVERGED, V_last
                V_previous = V_current                                               # :218
        return f, x, y, n, (CAP if force_steps is None else None), V_last

    def descend_all(self, q, f_lim, **kw):
        """descend() over seeds q [n, 3] -> (q [n, 3], steps [n], reasons, V [n])."""
        q = np.asarray(q, dtype=float).reshape(-1, 3)
        out = [self.descend(qi, f_lim, **kw) for qi in q]
        return (np.array([o[:3] for o in out]).reshape(-1, 3),
                np.array([o[3] for o in out], dtype=np.int64),
                [o[4] for o in out], np.array([o[5] for o in out]))
