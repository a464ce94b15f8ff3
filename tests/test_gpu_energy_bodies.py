"""Every kernel body of rhmc_energy, rhmc_gradient and rhmc_mh.

rhmc_energy launches one of 22 kernel bodies (csrc/rhmc_launch.hpp:
launch_energy, launch_energy_slotted), rhmc_gradient
one of 16 (launch_gradient), each computing dVdq (kind 0) or dphidq (kind 1),
and rhmc_mh one of 8 fused bodies (launch_mh_k1, launch_mh_pk) or the
four-kernel loop in its two forms (run_mh: one thread per chain below 8 stars,
one wave per chain from 8).  TABLE_E, TABLE_G and TABLE_MH hold at least one
shape per body with the body's key beside it; tests/test_energy_bodies.py
checks on the CPU (tests/native/traj_bodies.cpp in its `energy`, `gradient`
and `mh` modes, which ask csrc/rhmc_select.hpp and the launchers' own
csrc/rhmc_dispatch.hpp) that every shape is served by the body written here at
every chain count launched below, and that the tables cover every body.  Images
and starts come from test_gpu_rhmc_diag._field; no golden is read.

Energy, each row against oracle.rhmc_ref.RefModel.V / .T (V at rtol 1e-12, T
at rtol 1e-12 and atol 1e-12, the bars of test_gpu_parity):

* `inside`: the prior off, and on under an explicit V_prior_const; p = None; a
  subset of the chains and one chain alone bit-identical to the batch.
* `support`: six chains.  Star K - 1 of chain 0 and star 0 of chain 1 sit 1 %
  below f_lim (inf under f_pos, finite without), chain 2 holds a flux exactly
  at f_lim (finite), chain 3 a star at x = -0.7 (a clamped window, finite),
  chain 4 a star exactly at x = -1 and one at y = cols + 1 (finite: the test
  is strict), chain 5 a star at x = -1.5 (inf; finite under pos_check=False,
  compared with _V_nocheck below, RefModel.V without its position check).
* `vc` (every body but regwin1, which the pair potential leaves): beta and
  Vc_r_pow of golden vc5; in chain 0 star K - 1 sits on star 1 (the
  R < 1e-10 -> 1e32 branch), in another slot wherever there are two.
* a NaN chain beside wave-mates (regwin1 only): the mates bit-identical.
* `ragged` (every body a ragged set can reach, rhmc_select.hpp's
  ragged_family: all but regwin1 and ldsimage/1): one energy_ragged_device
  call on star counts from the low end of the row's slot class to the row's K,
  rows permuted, ld > 3 K_max, bit-identical to the fixed-K calls; again
  with quiet NaNs past 3 K[row] and in the unused row, whose d_K is 0, then
  K_max + 1: V bit-identical (tests/test_gpu_ragged_bodies.py does the same
  to the step).
  test_gpu_ragged.test_ragged_equals_fixed_K (slotted/Dense32/1,
  slotted/WinGG/2, ldsimage/16) and test_gpu_hugek.
  test_hugek_ragged_equals_fixed_K (slotted/WinGG/8) do the same on their
  goldens; the rows here run all the same, on other shapes.

Gradient, each row, kind 0 and 1, against RefModel.dVdq / .dphidq: `inside`
with the prior off and on, `edge` (a star 0.3 px inside x = 0, one at
x = -0.7), `vc` with the coincident pair; subsets bit-identical.  The bar is
per element: |got_e - want_e| <= 1e-12 S_e with S_e = sum over pixels of
(D / Lambda + 1) |w_e PSF_k| plus the absolute prior, pair-potential and
metric terms (scale() below); w_e is 1, f (i - x + 1/2) / sigma^2 or
f (j - y + 1/2) / sigma^2.  The 1e-12 is derived: reordering a sum of
n = side^2 terms moves it by at most about 2 n 2^-53 of the sum of absolute
values, 9e-13 at 64 px, and the elementary functions add a few ulp per term.
The chain-scaled bar of test_gpu_parity (|g - want| / (max over the chain
|want| + 1) < 1e-10) is asserted as well; it is blind to a faint star's
component, whose S_e is about 1e-3 of the chain's largest gradient.

MH, one row per fused body and the loop at K = 3, 7, 8, 12, 70: host randoms,
4 iterations of 5 steps, f_pos, against test_gpu_mh_fused._oracle_mh: accept
sequences exact, E_chain at rtol 1e-11, the final q at 1e-9 of |value| + 1, a
subset bit-identical; the fused rows again under RHMC_OPT_MH_FUSED = 0 with
identical accepts.

conditions_e / _g / _mh assert on the CPU what the bars rest on
(tests/test_energy_bodies.py runs them for every row): the oracle lies within
a tenth of each bar of a np.longdouble restatement (_Ld below), no flux or
coordinate compared with the wall or the support lies within 1e-7 relative of
it (those placed exactly on it excepted), every |log u + dE| of an MH row is
at least 1e-6 and its chains hold an accept and a reject.  DESIGN section 4i
has the measured errors per body.
"""
import numpy as np
import pytest

from helpers import vprior_const
from oracle.rhmc_ref import RefModel, gauss_psf
from rhmc_amd import workloads
from rhmc_amd.photometry import default_exp_setup
from test_gpu_mh_fused import _oracle_mh
from test_gpu_rhmc_diag import _field

pytestmark = pytest.mark.gpu

REF_FWHM = default_exp_setup()[3]     # the reference PSF, 3.5 px
WIDE_FWHM = 3.8     # inside (3.555, 4.06]: the 32-px windows are unsupported by rule
V_RTOL, T_RTOL, T_ATOL = 1e-12, 1e-12, 1e-12
G_BAR, G_CHAIN_BAR = 1e-12, 1e-10
FMIN, FMAX = 1.0, 1e5       # the prior's flux range (V_prior_const)
VC_BETA, VC_POW = 0.01, 2.0     # golden vc5
N_ITER, N_STEPS = 4, 5
MH_E_RTOL, MH_Q_BAR, MH_MARGIN = 1e-11, 1e-9, 1e-6
LD = np.longdouble

# id: K, image side, chains, forced kernel, use_Vc, PSF FWHM, image exact in
# fp32 (else the same image + 0.1), body key
_COMMON = {
    # LDS image: no forcing needed, these two operations have no register
    # kernel for 2+ stars (nor, at 40 px, for one)
    "k1_lds40": (1, 40, 3, None, False, REF_FWHM, True, "ldsimage/1"),
    "k2_lds40": (2, 40, 5, None, False, REF_FWHM, True, "ldsimage/2"),
    "k3_lds40": (3, 40, 3, None, False, REF_FWHM, True, "ldsimage/4"),
    "k5_lds40": (5, 40, 2, None, False, REF_FWHM, True, "ldsimage/8"),
    "k9_lds40": (9, 40, 3, None, False, REF_FWHM, True, "ldsimage/16"),
    "k16_lds40": (16, 40, 5, None, False, REF_FWHM, False, "ldsimage/16"),
    "k1_vc48": (1, 48, 3, None, True, REF_FWHM, True, "ldsimage/1"),
    "k2_wide40": (2, 40, 3, None, False, WIDE_FWHM, True, "ldsimage/2"),
    # the shapes on which a ragged set reaches the LDS-image energy (the
    # pixel-major step's energy: 2-10 stars on 32/48-px fp32-exact images)
    "k2_lds32": (2, 32, 3, None, False, REF_FWHM, True, "ldsimage/2"),
    "k4_lds48": (4, 48, 2, None, False, REF_FWHM, True, "ldsimage/4"),
    "k8_lds32": (8, 32, 3, None, False, REF_FWHM, True, "ldsimage/8"),
    "k10_lds48": (10, 48, 5, None, False, REF_FWHM, True, "ldsimage/16"),
    # windowed, one slot: by rule, and forced
    "k40_win64": (40, 64, 3, None, False, REF_FWHM, True, "slotted/Win*/1"),
    "k12_windowed": (12, 32, 5, "windowed", False, REF_FWHM, True, "slotted/Win*/1"),
    "k64_windowed": (64, 48, 2, "windowed", False, REF_FWHM, False, "slotted/Win*/1"),
    # the star counts of test_gpu_step_bodies.TABLE: a last slot nearly empty,
    # a whole slot empty, all slots full
    "k70_wingg2": (70, 64, 3, None, False, REF_FWHM, True, "slotted/WinGG/2"),
    "k130_wingg4": (130, 64, 2, None, False, REF_FWHM, True, "slotted/WinGG/4"),
    "k260_wingg8": (260, 32, 2, "windowed", False, REF_FWHM, True, "slotted/WinGG/8"),
    "k520_wingg16": (520, 32, 3, "windowed", False, REF_FWHM, True, "slotted/WinGG/16"),
    "k1024_wingg16": (1024, 32, 2, "windowed", False, REF_FWHM, True, "slotted/WinGG/16"),
    "k12_dense32": (12, 32, 5, None, False, REF_FWHM, True, "slotted/Dense32/1"),
    "k70_dense32": (70, 32, 3, None, False, REF_FWHM, True, "slotted/Dense32/2"),
    "k256_dense32": (256, 32, 2, None, False, REF_FWHM, True, "slotted/Dense32/4"),
    "k12_dense48": (12, 48, 3, None, False, REF_FWHM, False, "slotted/Dense48/1"),
    "k70_dense48": (70, 48, 2, None, False, REF_FWHM, True, "slotted/Dense48/2"),
    "k129_dense48": (129, 48, 3, None, False, REF_FWHM, True, "slotted/Dense48/4"),
}
# one star, register window (energy, MH): 5 chains are one full wave and a
# one-chain wave, 17 chains (48 px, fp32) a second workgroup, partly filled
_REGWIN = {}
for _side in (32, 48, 64):
    for _f32 in (True, False):
        _REGWIN["k1_regwin%d_%s" % (_side, "f32" if _f32 else "f64")] = (
            1, _side, 17 if (_side, _f32) == (48, True) else 5, None, False, REF_FWHM, _f32,
            "regwin1/%d/%s" % (_side, "float" if _f32 else "double"))
TABLE_E = dict(_REGWIN)
TABLE_E.update({k: v[:7] + (v[7].replace("Win*", "WinEG"),) for k, v in _COMMON.items()})
TABLE_G = {k: v[:7] + (v[7].replace("Win*", "WinG"),) for k, v in _COMMON.items()}
NAN_ROWS = list(_REGWIN)
VC_ROWS = list(_COMMON)
# the lowest star count of the row's slot class that shares the row's ragged family
RAGGED_ROWS = {"k2_lds32": 2, "k4_lds48": 3, "k8_lds32": 5, "k10_lds48": 9, "k12_windowed": 2,
               "k64_windowed": 2, "k70_wingg2": 65, "k130_wingg4": 129, "k260_wingg8": 257,
               "k520_wingg16": 513, "k1024_wingg16": 513, "k12_dense32": 11, "k70_dense32": 65,
               "k256_dense32": 129, "k12_dense48": 11, "k70_dense48": 65, "k129_dense48": 129}

# id: K, image side, chains, forced kernel, RHMC_OPT_MH_FUSED, PSF FWHM, image
# exact in fp32, body key, the body under RHMC_OPT_MH_FUSED = 0 (or None), dt
TABLE_MH = {}
for _name, _row in _REGWIN.items():
    TABLE_MH[_name] = _row[:4] + (1,) + _row[5:7] + ("mh/" + _row[7], "mh/loop/thread", 0.3)
TABLE_MH.update({
    "k3_pixmajor32": (3, 32, 5, None, 1, REF_FWHM, True, "mh/pixmajor/32", "mh/loop/thread", 0.3),
    "k10_pixmajor48": (10, 48, 3, None, 1, REF_FWHM, True, "mh/pixmajor/48", "mh/loop/wave", 0.3),
    # the loop: thread form, both sides of the K >= 8 switch, 3 K > 64 coordinates
    "k3_loop40": (3, 40, 5, None, 1, REF_FWHM, True, "mh/loop/thread", None, 0.3),
    "k7_loop40": (7, 40, 3, None, 1, REF_FWHM, True, "mh/loop/thread", None, 0.3),
    "k8_loop40": (8, 40, 5, None, 1, REF_FWHM, True, "mh/loop/wave", None, 0.3),
    "k12_loop32": (12, 32, 3, None, 1, REF_FWHM, True, "mh/loop/wave", None, 0.3),
    "k70_loop48": (70, 48, 2, None, 1, REF_FWHM, True, "mh/loop/wave", None, 0.3),
})
N_SUPPORT = 6       # chains of the `support` scenario
N_RAGGED = 5        # chains of the ragged set
_cache = {}


def _subset(n):
    return [0, n - 1] if n > 2 else [n - 1]


def launch_counts(op, name):
    """Every chain count the tests below launch for a row."""
    n = {"energy": TABLE_E, "gradient": TABLE_G, "mh": TABLE_MH}[op][name][2]
    counts = {n, len(_subset(n)), 1}
    if op == "energy":
        counts |= {N_SUPPORT, N_RAGGED}
    return sorted(counts)


# ---------------------------------------------------------------- the inputs
def _par(side, fwhm, prior=False, use_Vc=False, dt=0.1):
    """rhmc_params of one run (capi.make_params' keywords)."""
    par, _ = workloads.base_params(dt, g_xx=0.05, g_ff=4., g_ff2=4., use_prior=prior, alpha=2.)
    assert par["fwhm_pix"] == REF_FWHM
    par.update(fwhm_pix=fwhm, use_Vc=use_Vc, beta=VC_BETA, Vc_r_pow=VC_POW)
    if prior:
        par["V_prior_const"] = vprior_const(dict(par, rows=side, cols=side, fmin=FMIN, fmax=FMAX))
    return par


def _model(side, D, par, cls=RefModel):
    return cls(D, dict(par, rows=side, cols=side, fmin=FMIN, fmax=FMAX))


def _start(row):
    K, side, n, f32 = row[0], row[1], row[2], row[6]
    D, q0, z = _field(K, side, n, 100 + K + side)
    if not f32:
        D = D + 0.1
    assert np.array_equal(D, D.astype(np.float32).astype(float)) == f32
    return D, q0, z


def _coincide(q0, K):
    """Star K - 1 of chain 0 onto star 1 (star 0 where there are two): another
    slot wherever the kernel has two."""
    if K >= 2:
        a = 1 if K > 2 else 0
        q0[0, 3 * (K - 1) + 1: 3 * K] = q0[0, 3 * a + 1: 3 * a + 3]
        assert (K - 1) // 64 != a // 64 or K <= 64
    return q0


def _V_nocheck(m, q, f_pos=False):
    """RefModel.V (sampler_RHMC.py:294-351) without its position check, which
    RefModel.V always makes and rhmc_energy drops under RHMC_V_NO_POSCHECK."""
    P, K = m.p, q.size // 3
    if f_pos and (q[0::3] < P["f_lim"]).any():
        return np.inf
    Lam = np.ones_like(m.D) * P["B_count"]
    for i in range(K):
        Lam += q[3 * i] * gauss_psf(m.rows, m.cols, q[3 * i + 1], q[3 * i + 2], P["fwhm_pix"])
    V = np.sum(Lam - m.D * np.log(Lam))
    if P["use_prior"]:
        V += sum(P["alpha"] * np.log(f) + vprior_const(P) for f in q[0::3])
    if P["use_Vc"]:
        X, Y = q[1::3], q[2::3]
        R = np.sqrt((X - X.reshape((K, 1))) ** 2 + (Y - Y.reshape((K, 1))) ** 2)
        R[np.abs(R) < 1e-10] = 1e32
        V += 0.5 * P["beta"] * np.sum((1. / R) ** P["Vc_r_pow"])
    return V


# ----------------------------------------- the np.longdouble restatement, S_e
class _Ld:
    """V, T and the gradients of one chain in np.longdouble, with the PSF as the
    product of its two one-dimensional factors; the model's constants (sigma,
    2 sigma^2, the normalisation) are the oracle's doubles."""

    def __init__(self, D, par, side, q, dtype=LD):
        t = self.t = dtype
        self.par, self.K, self.D = par, q.size // 3, np.asarray(D).astype(t)
        sigma = par["fwhm_pix"] / 2.354
        self.var = t(sigma ** 2)
        two, norm = t(2 * sigma ** 2), t(np.pi * 2 * sigma ** 2)
        self.f, self.x, self.y = (q[i::3].astype(t) for i in range(3))
        c = np.arange(side).astype(t) + t(0.5)
        self.dx, self.dy = c[None, :] - self.x[:, None], c[None, :] - self.y[:, None]
        self.ex = np.exp(-self.dx * self.dx / two) / norm
        self.ey = np.exp(-self.dy * self.dy / two)
        self.Lam = t(par["B_count"]) + np.einsum("k,ki,kj->ij", self.f, self.ex, self.ey)

    def _R(self):
        X, Y = self.x, self.y
        R = np.sqrt((X[None, :] - X[:, None]) ** 2 + (Y[None, :] - Y[:, None]) ** 2)
        R[np.abs(R) < 1e-10] = self.t(1e32)
        return R

    def _metric(self):
        """H_ff, H_xx and their flux derivatives (sampler_RHMC.py:260-292)."""
        P, t, f = self.par, self.t, self.f
        B, g0, g1, g2 = t(P["B_count"]), t(P["g0"]), t(P["g1"]), t(P["g2"])
        low = f < P["f_low"]
        fc = np.where(low, t(P["f_low"]), f)
        a = 1 / (g1 * fc) + B / (g2 * fc ** 2)
        hxx = t(P["g_xx"]) / a
        hxx_g = np.where(low, t(0), t(P["g_xx"]) * (1 / (g1 * fc ** 2) + 2 * B / (g2 * fc ** 3))
                         / a ** 2)
        hff = 1 / (f / t(P["g_ff2"]) + (B / g0) / t(P["g_ff"]))
        hff_g = -1 / (f + (B / g0) / t(P["g_ff"])) ** 2
        return hff, hff_g, hxx, hxx_g

    def V(self):
        P = self.par
        V = np.sum(self.Lam - self.D * np.log(self.Lam))
        if P["use_prior"]:
            V += np.sum(self.t(P["alpha"]) * np.log(self.f) + self.t(P["V_prior_const"]))
        if P["use_Vc"]:
            V += self.t(0.5 * P["beta"]) * np.sum((1 / self._R()) ** self.t(P["Vc_r_pow"]))
        return V

    def T(self, p):
        hff, _, hxx, _ = self._metric()
        p = p.astype(self.t)
        return (np.sum(p[0::3] ** 2 / hff + (p[1::3] ** 2 + p[2::3] ** 2) / hxx)
                + np.sum(np.log(np.abs(hff)) + 2 * np.log(np.abs(hxx)))) / 2

    def _terms(self, kind):
        """Per element [3K]: the pixel sum's weights (wx [K, side], wy [K, side])
        and the terms added after it."""
        P, t, K = self.par, self.t, self.K
        fv = self.f / self.var
        wx = [self.ex, fv[:, None] * self.dx * self.ex, fv[:, None] * self.ex]
        wy = [self.ey, self.ey, self.dy * self.ey]
        extra = [[] for _ in range(3)]
        if P["use_prior"]:
            extra[0].append(t(P["alpha"]) / self.f)
        if P["use_Vc"]:
            r = (1 / self._R()) ** t(P["Vc_r_pow"] + 2) * t(P["beta"] * P["Vc_r_pow"])
            extra[1].append(r * (self.x[None, :] - self.x[:, None]))     # [K, K], summed over j
            extra[2].append(r * (self.y[None, :] - self.y[:, None]))
        if kind == 1:
            hff, hff_g, hxx, hxx_g = self._metric()
            extra[0] += [hff_g / hff / 2, hxx_g / hxx]
        return wx, wy, extra

    def gradient(self, kind, absolute=False):
        """dVdq (kind 0) or dphidq (kind 1) [3K]; absolute: S_e, the same sums
        over absolute values with D / Lambda + 1 for D / Lambda - 1."""
        wx, wy, extra = self._terms(kind)
        rho = self.D / self.Lam + 1 if absolute else self.D / self.Lam - 1
        out = np.zeros(3 * self.K, self.t)
        for e in range(3):
            a, b = (np.abs(wx[e]), np.abs(wy[e])) if absolute else (wx[e], wy[e])
            s = np.sum((a @ rho) * b, axis=1)
            out[e::3] = s if absolute else -s
            for term in extra[e]:
                term = np.abs(term) if absolute else term
                out[e::3] += term.sum(axis=1) if term.ndim == 2 else term
        return out


def scale(D, par, side, q, kind):
    """S_e of one chain [3K], in fp64."""
    return _Ld(D, par, side, q, np.float64).gradient(kind, absolute=True)


def _clearance(q, side, f_lim):
    """The least relative distance of a flux from f_lim and of a coordinate
    from the support's edges, values exactly on them left out."""
    f, xy = q[..., 0::3].ravel(), np.concatenate([q[..., 1::3].ravel(), q[..., 2::3].ravel()])
    d = np.concatenate([np.abs(f / f_lim - 1.), np.abs(xy + 1.) / (side + 1.),
                        np.abs(xy - (side + 1.)) / (side + 1.)])
    return float(d[d > 0].min())


# ------------------------------------------------------------------ energy
def energy_case(name, scen):
    """dict of D, side, the runs [(par, q, p, f_pos, pos_check, want V, want T)]."""
    if ("e", name, scen) in _cache:
        return _cache[("e", name, scen)]
    K, side, n, _, use_Vc, fwhm, _, _ = TABLE_E[name]
    D, q0, z = _start(TABLE_E[name])
    runs = []

    def add(par, q, p, f_pos, pos_check):
        m = _model(side, D, par)
        V = np.array([m.V(r, f_pos) if pos_check else _V_nocheck(m, r, f_pos) for r in q])
        T = None if p is None else np.array([m.T(pc, m.H(r)) for r, pc in zip(q, p)])
        runs.append(dict(par=par, q=q, p=p, f_pos=f_pos, pos_check=pos_check, V=V, T=T))

    if scen == "inside":
        for prior in (False, True):
            par = _par(side, fwhm, prior, use_Vc)
            p0 = z * np.sqrt(np.array([_model(side, D, par).H(r) for r in q0]))
            add(par, q0, p0, False, True)
        assert all(np.isfinite(r["V"]).all() for r in runs)
    elif scen == "vc":
        par = _par(side, fwhm, False, True)
        add(par, _coincide(q0.copy(), K), None, False, True)
        assert np.isfinite(runs[0]["V"]).all()
    else:
        par = _par(side, fwhm, False, use_Vc)
        f_lim = par["f_lim"]
        q = q0[np.arange(N_SUPPORT) % n].copy()
        mid = 3 * (K // 2)
        q[0, 3 * (K - 1)] = 0.99 * f_lim
        q[1, 0] = 0.99 * f_lim
        q[2, mid] = f_lim
        q[3, mid + 1] = -0.7
        q[4, 1] = -1.0
        q[4, 3 * (K - 1) + 2] = side + 1.0
        q[5, 3 * (K - 1) + 1] = -1.5
        add(par, q, None, True, True)
        add(par, q, None, False, True)
        add(par, q, None, False, False)
        fin = np.isfinite([r["V"] for r in runs])
        assert np.array_equal(fin, [[0, 0, 1, 1, 1, 0], [1, 1, 1, 1, 1, 0], [1] * 6]), (name, fin)
    out = dict(D=D, side=side, runs=runs)
    _cache[("e", name, scen)] = out
    return out


def _scenarios_e(name):
    return ["inside", "support"] + (["vc"] if name in VC_ROWS else [])


def conditions_e(name):
    """{scenario: (V oracle against longdouble as a fraction of the bar, T the
    same, the least clearance from the wall and the support)}."""
    out = {}
    for scen in _scenarios_e(name):
        case = energy_case(name, scen)
        eV = eT = 0.
        clear = np.inf
        for r in case["runs"]:
            clear = min(clear, _clearance(r["q"], case["side"], r["par"]["f_lim"]))
            for c, q in enumerate(r["q"]):
                if not np.isfinite(r["V"][c]):
                    continue
                ld = _Ld(case["D"], r["par"], case["side"], q)
                V = ld.V()
                eV = max(eV, float(abs(r["V"][c] - V) / abs(V)) / V_RTOL)
                if r["T"] is not None:
                    T = ld.T(r["p"][c])
                    eT = max(eT, float(abs(r["T"][c] - T) / (T_ATOL + T_RTOL * abs(T))))
        assert eV <= 0.1 and eT <= 0.1 and clear > 1e-7, (name, scen, eV, eT, clear)
        out[scen] = (eV, eT, clear)
    return out


# ---------------------------------------------------------------- gradient
class _Once(RefModel):
    """RefModel whose dphidq reuses the dVdq just computed for the same q."""
    _key = None

    def dVdq(self, q):
        if self._key != q.tobytes():
            self._key, self._g = q.tobytes(), RefModel.dVdq(self, q)
        return self._g.copy()


def gradient_case(name, scen):
    """dict of D, side, the runs [(par, q, {kind: (want, S_e)})]."""
    if ("g", name, scen) in _cache:
        return _cache[("g", name, scen)]
    K, side, n, _, use_Vc, fwhm, _, _ = TABLE_G[name]
    D, q0, _ = _start(TABLE_G[name])
    runs = []

    def add(par, q):
        m = _model(side, D, par, _Once)
        both = [(m.dVdq(r), m.dphidq(r)) for r in q]
        want = {k: np.array([b[k] for b in both]) for k in (0, 1)}
        S = {k: np.array([scale(D, par, side, r, k) for r in q]) for k in (0, 1)}
        runs.append(dict(par=par, q=q, want=want, S=S))

    if scen == "inside":
        for prior in (False, True):
            add(_par(side, fwhm, prior, use_Vc), q0)
    elif scen == "edge":
        q = q0.copy()
        q[0, 3 * (K - 1) + 1] = 0.3
        q[n - 1, 1] = -0.7
        add(_par(side, fwhm, True, use_Vc), q)
    else:
        add(_par(side, fwhm, False, True), _coincide(q0.copy(), K))
    out = dict(D=D, side=side, runs=runs)
    _cache[("g", name, scen)] = out
    return out


def conditions_g(name):
    """{scenario: the oracle's gradient against longdouble as a fraction of the
    per-element bar}."""
    out = {}
    for scen in ("inside", "edge", "vc"):
        case = gradient_case(name, scen)
        worst = 0.
        for r in case["runs"]:
            for c, q in enumerate(r["q"]):
                ld = _Ld(case["D"], r["par"], case["side"], q)
                for kind in (0, 1):
                    err = np.abs(r["want"][kind][c] - ld.gradient(kind)) / r["S"][kind][c]
                    worst = max(worst, float(err.max()) / G_BAR)
        assert worst <= 0.1, (name, scen, worst)
        out[scen] = worst
    return out


# ---------------------------------------------------------------------- MH
class _Recording(RefModel):
    """RefModel that keeps what V and T returned, in call order."""

    def __init__(self, D, par):
        RefModel.__init__(self, D, par)
        self.Vs, self.Ts = [], []

    def V(self, q, f_pos=False):
        self.Vs.append(RefModel.V(self, q, f_pos))
        return self.Vs[-1]

    def T(self, p, H_diag):
        self.Ts.append(RefModel.T(p, H_diag))
        return self.Ts[-1]


def mh_case(name):
    """The oracle's chains of a row: D, par, q0, z, u, per chain the final q,
    the accepts and E_chain, the least |log u + dE|."""
    if ("mh", name) in _cache:
        return _cache[("mh", name)]
    K, side, n, _, _, fwhm, _, _, _, dt = TABLE_MH[name]
    D, q0, _ = _start(TABLE_MH[name])
    rng = np.random.RandomState(7 + K + side)
    z = rng.randn(N_ITER, n, 3 * K)
    u = rng.uniform(size=(N_ITER, n))
    par = _par(side, fwhm, dt=dt)
    q, acc, E, margin = [], [], [], np.inf
    for c in range(n):
        m = _model(side, D, par, _Recording)
        qo, ao, Eo = _oracle_mh(m, q0[c], z[:, c], u[:, c], N_STEPS, par["f_lim"])
        assert len(m.Vs) == N_ITER + 1 and len(m.Ts) == 2 * N_ITER
        dE = np.array(m.Vs[1:]) + np.array(m.Ts[1::2]) - Eo
        assert np.array_equal(ao, (dE < 0) | (np.log(u[:, c]) < -dE))
        margin = min(margin, float(np.abs(np.log(u[:, c]) + dE).min()))
        q.append(qo)
        acc.append(ao)
        E.append(Eo)
    out = dict(D=D, par=par, q0=q0, z=z, u=u, q=np.array(q), acc=np.array(acc).T,
               E=np.array(E).T, margin=margin)
    _cache[("mh", name)] = out
    return out


def conditions_mh(name):
    """(the least |log u + dE|, the accepted fraction)."""
    case = mh_case(name)
    assert case["margin"] >= MH_MARGIN, (name, case["margin"])
    assert case["acc"].any() and not case["acc"].all(), (name, case["acc"])
    assert np.isfinite(case["E"]).all()
    return case["margin"], float(case["acc"].mean())


# ------------------------------------------------------------------- the GPU
class _Ctx:
    """A context on an image with the row's forced kernel."""

    def __init__(self, capi, D, kernel):
        self.ctx = capi.Context(D, kernel=kernel or "auto")

    def __enter__(self):
        return self.ctx

    def __exit__(self, *exc):
        self.ctx.close()
        return False


def _rel(got, want):
    return float(np.max(np.abs(got - want) / np.abs(want))) if len(want) else 0.


def _check_energy(ctx, capi, r, n_sub=True):
    """One run against the oracle at the bars; the subsets bit-identical.
    Returns the worst relative error of V, the worst error of T as a fraction
    of its bar, V and T."""
    P = capi.make_params(**r["par"])
    V, T = ctx.energy(P, r["q"], r["p"], f_pos=r["f_pos"], pos_check=r["pos_check"])
    fin = np.isfinite(r["V"])
    assert np.array_equal(np.isposinf(V), ~fin) and np.array_equal(np.isfinite(V), fin), (V, r["V"])
    eV, eT = _rel(V[fin], r["V"][fin]), 0.
    if r["p"] is None:
        assert T is None
    else:
        eT = float(np.max(np.abs(T - r["T"]) / (T_ATOL + T_RTOL * np.abs(r["T"]))))
        V2, T2 = ctx.energy(P, r["q"], None, f_pos=r["f_pos"], pos_check=r["pos_check"])
        assert T2 is None
        np.testing.assert_allclose(V2, r["V"], rtol=V_RTOL, atol=0.)
    n = len(r["q"])
    for sub in (_subset(n), [n - 1]) if n_sub else ():
        Vs, Ts = ctx.energy(P, r["q"][sub], None if r["p"] is None else r["p"][sub],
                            f_pos=r["f_pos"], pos_check=r["pos_check"])
        assert np.array_equal(Vs, V[sub]) and (T is None or np.array_equal(Ts, T[sub]))
    return eV, eT, V, T


def _report(capsys, op, name, body, text):
    with capsys.disabled():
        print("\n  %s %s [%s]: %s" % (op, name, body, text))


@pytest.mark.parametrize("name", list(TABLE_E))
def test_energy_inside(gpu_lib, name, capsys):
    capi = gpu_lib
    case = energy_case(name, "inside")
    worst = []
    with _Ctx(capi, case["D"], TABLE_E[name][3]) as ctx:
        for r in case["runs"]:
            eV, eT, V, T = _check_energy(ctx, capi, r)
            worst.append((eV, eT))
            np.testing.assert_allclose(V, r["V"], rtol=V_RTOL, atol=0.)
            np.testing.assert_allclose(T, r["T"], rtol=T_RTOL, atol=T_ATOL)
    _report(capsys, "energy", name, TABLE_E[name][7], "V %.2g, %.2g with the prior (rtol 1e-12); "
            "T %.2g of its bar" % (worst[0][0], worst[1][0], max(w[1] for w in worst)))


@pytest.mark.parametrize("name", list(TABLE_E))
def test_energy_support(gpu_lib, name, capsys):
    capi = gpu_lib
    case = energy_case(name, "support")
    worst = 0.
    with _Ctx(capi, case["D"], TABLE_E[name][3]) as ctx:
        for r in case["runs"]:
            eV, _, V, _ = _check_energy(ctx, capi, r, n_sub=False)
            worst = max(worst, eV)
            fin = np.isfinite(r["V"])
            np.testing.assert_allclose(V[fin], r["V"][fin], rtol=V_RTOL, atol=0.)
    _report(capsys, "energy", name, TABLE_E[name][7], "support V %.2g" % worst)


@pytest.mark.parametrize("name", VC_ROWS)
def test_energy_pair_potential(gpu_lib, name, capsys):
    capi = gpu_lib
    case = energy_case(name, "vc")
    with _Ctx(capi, case["D"], TABLE_E[name][3]) as ctx:
        eV, _, V, _ = _check_energy(ctx, capi, case["runs"][0])
        np.testing.assert_allclose(V, case["runs"][0]["V"], rtol=V_RTOL, atol=0.)
    _report(capsys, "energy", name, TABLE_E[name][7], "pair potential V %.2g" % eV)


@pytest.mark.parametrize("name", NAN_ROWS)
def test_energy_nan_chain_beside_wave_mates(gpu_lib, name):
    """Chain 1 holds a NaN: its wave-mates' V and T as without it."""
    capi = gpu_lib
    case = energy_case(name, "inside")
    r = case["runs"][0]
    P = capi.make_params(**r["par"])
    qb = r["q"].copy()
    qb[1, 1] = np.nan
    with _Ctx(capi, case["D"], TABLE_E[name][3]) as ctx:
        V, T = ctx.energy(P, r["q"], r["p"])
        V2, T2 = ctx.energy(P, qb, r["p"])
    others = [c for c in range(len(qb)) if c != 1]
    assert not np.isfinite(V2[1])
    assert np.array_equal(V2[others], V[others]) and np.array_equal(T2[others], T[others])


@pytest.mark.parametrize("name", list(RAGGED_ROWS))
def test_energy_ragged_equals_fixed_K(gpu_lib, name):
    import torch
    capi = gpu_lib
    K, side, _, kernel, use_Vc, fwhm, _, _ = TABLE_E[name]
    lo = RAGGED_ROWS[name]
    Ks = [lo, K, (lo + K) // 2, K, lo][:N_RAGGED]
    D, q0, _ = _start(TABLE_E[name])
    ld = 3 * K + 7
    q = np.zeros((N_RAGGED + 1, ld))
    order = np.random.RandomState(K).permutation(N_RAGGED + 1)[:N_RAGGED]   # one row unused
    for j, r in enumerate(order):
        q[r, :3 * Ks[j]] = q0[j % len(q0), :3 * Ks[j]]
    K_of = np.zeros(N_RAGGED + 1, np.int32)
    K_of[order] = Ks
    par = _par(side, fwhm, True, use_Vc)
    P = capi.make_params(**par)
    dev = torch.device("cuda:0")
    with _Ctx(capi, D, kernel) as ctx:
        for k in range(lo, K + 1):
            assert ctx.ragged_ok(P, k), k
        qd = torch.from_numpy(q).to(dev)
        Kd = torch.from_numpy(K_of).to(dev)
        rows = torch.from_numpy(order.astype(np.int64)).to(dev)
        Vd = torch.zeros(N_RAGGED, dtype=torch.float64, device=dev)
        ctx.energy_ragged_device(P, qd.data_ptr(), ld, rows.data_ptr(), Kd.data_ptr(), N_RAGGED,
                                 min(Ks), max(Ks), capi.V_FLUX_WALL, Vd.data_ptr())
        torch.cuda.synchronize()
        Vg = Vd.cpu().numpy()
        assert np.isfinite(Vg).all()
        for k in sorted(set(Ks)):
            js = [j for j in range(N_RAGGED) if Ks[j] == k]
            V, _ = ctx.energy(P, q[order[js], :3 * k], None, f_pos=True)
            assert np.array_equal(Vg[js], V), (k, Vg[js], V)
        # hostile padding: quiet NaNs of a known payload past 3 K[row] and in
        # the unused row, whose d_K is 0, then K_max + 1 (0 would fault or
        # corrupt if read, K_max + 1 computes on the poison): V bit-identical
        unused = sorted(set(range(N_RAGGED + 1)) - set(order))
        for bad_K in (0, K + 1):
            qh = np.full(q.shape, 0x7FF8DEAD0000BEEF, np.uint64).view(np.float64)
            for j, r in enumerate(order):
                qh[r, :3 * Ks[j]] = q[r, :3 * Ks[j]]
            assert np.isnan(qh[unused]).all() and np.isnan(qh[order[0], 3 * Ks[0]:]).all()
            Kh = K_of.copy()
            Kh[unused] = bad_K
            qhd = torch.from_numpy(qh).to(dev)
            Khd = torch.from_numpy(Kh).to(dev)
            Vh = torch.zeros(N_RAGGED, dtype=torch.float64, device=dev)
            ctx.energy_ragged_device(P, qhd.data_ptr(), ld, rows.data_ptr(), Khd.data_ptr(),
                                     N_RAGGED, min(Ks), max(Ks), capi.V_FLUX_WALL, Vh.data_ptr())
            torch.cuda.synchronize()
            assert np.array_equal(Vh.cpu().numpy(), Vg), (bad_K, Vh.cpu().numpy(), Vg)
            assert np.array_equal(qhd.cpu().numpy().view(np.uint64), qh.view(np.uint64))


def _check_gradient(ctx, capi, r):
    """Both kinds of one run; returns the worst error as a fraction of S_e and
    of the chain's scale."""
    P = capi.make_params(**r["par"])
    n = len(r["q"])
    worst = [0., 0.]
    for kind in (0, 1):
        g = ctx.gradient(P, r["q"], kind=kind)
        want, S = r["want"][kind], r["S"][kind]
        for sub in (_subset(n), [n - 1]):
            assert np.array_equal(ctx.gradient(P, r["q"][sub], kind=kind), g[sub])
        err = np.abs(g - want)
        worst[0] = max(worst[0], float((err / S).max()))
        chain = np.abs(want).max(axis=1, keepdims=True) + 1.
        worst[1] = max(worst[1], float((err / chain).max()))
        assert np.isfinite(g).all()
    return worst


@pytest.mark.parametrize("scen", ["inside", "edge", "vc"])
@pytest.mark.parametrize("name", list(TABLE_G))
def test_gradient(gpu_lib, name, scen, capsys):
    capi = gpu_lib
    case = gradient_case(name, scen)
    worst = [0., 0.]
    with _Ctx(capi, case["D"], TABLE_G[name][3]) as ctx:
        for r in case["runs"]:
            worst = [max(a, b) for a, b in zip(worst, _check_gradient(ctx, capi, r))]
    _report(capsys, "gradient", name, TABLE_G[name][7], "%s: %.2g of S_e (bar 1e-12), %.2g of the "
            "chain's scale (1e-10)" % (scen, worst[0], worst[1]))
    assert worst[0] <= G_BAR
    assert worst[1] < G_CHAIN_BAR


def _mh(ctx, capi, case, chains, fused):
    ctx.set_option(capi.OPT_MH_FUSED, int(fused))
    try:
        return ctx.mh(capi.make_params(**case["par"]), case["q0"][chains], N_ITER, N_STEPS,
                      f_pos=True, z=case["z"][:, chains], u=case["u"][:, chains])
    finally:
        ctx.set_option(capi.OPT_MH_FUSED, 1)


@pytest.mark.parametrize("name", list(TABLE_MH))
def test_mh(gpu_lib, name, capsys):
    capi = gpu_lib
    case = mh_case(name)
    n = len(case["q0"])
    with _Ctx(capi, case["D"], TABLE_MH[name][3]) as ctx:
        out = _mh(ctx, capi, case, list(range(n)), True)
        sub = _subset(n)
        part = _mh(ctx, capi, case, sub, True)
        loop = _mh(ctx, capi, case, list(range(n)), False) if TABLE_MH[name][8] else None
    assert np.array_equal(out["accept"].astype(bool), case["acc"])
    eE = _rel(out["E_chain"], case["E"])
    eq = float((np.abs(out["q"] - case["q"]) / (np.abs(case["q"]) + 1.)).max())
    _report(capsys, "mh", name, TABLE_MH[name][7], "E_chain %.2g (rtol 1e-11), q %.2g (1e-9), "
            "least |log u + dE| %.2g, accepted %.2f" % (eE, eq, case["margin"],
                                                         case["acc"].mean()))
    assert eE <= MH_E_RTOL and eq <= MH_Q_BAR
    for k in ("accept", "q", "E_chain", "q_chain"):
        assert np.array_equal(part[k], out[k][sub] if k == "q" else out[k][:, sub]), k
    if loop is not None:        # the four-kernel loop on the fused row's chains
        assert np.array_equal(loop["accept"], out["accept"])
        assert _rel(loop["E_chain"], case["E"]) <= MH_E_RTOL
        assert float((np.abs(loop["q"] - case["q"]) / (np.abs(case["q"]) + 1.)).max()) <= MH_Q_BAR
