"""Every kernel body of the implicit generalized-leapfrog step.

rhmc_leapfrog (Op::Step) launches one of 64 kernel bodies
(csrc/rhmc_launch.hpp: launch_leapfrog and its helpers).  TABLE holds at least
one shape per body with the body's key beside it; tests/test_step_bodies.py
checks on the CPU (tests/native/traj_bodies.cpp in its `step` mode, which asks
csrc/rhmc_select.hpp and the launchers' own csrc/rhmc_dispatch.hpp) that every
shape is served by the body written here at every chain count launched below,
and that the table covers all 64.

Each row runs, against oracle.rhmc_ref.RefModel.step stepped in Python:

* `free`: the flux prior on, no flux wall.  Every step from the oracle's own
  previous state, one launch per step: q to 1e-11 and p to 1e-10 of
  |value| + 1, the fixed-point counts exact (the bars of
  test_gpu_parity.test_trajectory_stepwise); all steps in one launch: 1e-9 /
  1e-8, summed counts and the status word exact (test_trajectory_fused); the
  same steps in two launches, a subset of the chains and one chain alone:
  bit-identical.
* `edge`: chain 0 starts 0.3 px inside x = 0 (its last star), the last chain
  0.3 px inside y = side - 1 (its first star), both moving outwards half a
  pixel per step: STATUS_REFLECT_XY exactly where the oracle reflects,
  STATUS_NEAR_WALL nowhere.
* `wall`: no prior, the wall at WALL_MAG.  Star K - 1 of even chains and star
  0 of odd chains starts 2 % and more above the wall with the momentum that
  takes it below on a chosen step (the latest of 3, 2, 1 that all chains of
  the launch can be aimed at: at dt = 0.1 the pull back up leaves only step
  1); one launch ends the even chains ON that step, a second ends the odd
  chains four steps (two from 65 stars) past theirs.
* `cap` (one row per family): counter_max = 2, ten times the step and
  delta = 1e-10, so that both fixed-point loops stop at the cap, two steps;
  STATUS_PLOOP_CAP / STATUS_QLOOP_CAP exact, each step from the oracle's
  state at the stepwise bar (the oracle takes the same capped iterates), both
  in one launch at the fused bar.
* A NaN chain beside wave-mates in the bodies that share a wave among chains.

The bars are conditional on the shape, and conditions() asserts the
conditions on the CPU (tests/test_step_bodies.py runs it for every row
without a GPU): every fixed-point test value the oracle records lies outside
delta (1 +- 1e-9) (DESIGN section 8 allows one iteration of difference inside
that band); no flux or coordinate compared with a wall lies within 1e-7
relative of it; and replaying each chain with dphidq scaled by 1 +- 1e-13
moves the end state by at most a tenth of the bar and changes no count or
flag.  Measured on an MI355X: every body within 2.5e-14 (q) / 1.7e-13 (p) per
step and 6.3e-14 / 2.5e-13 over a launch (DESIGN section 4f has the table per
body); no body takes a looser bar.
"""
import time

import numpy as np
import pytest

from oracle.rhmc_ref import RefModel
from rhmc_amd import workloads
from rhmc_amd.photometry import default_exp_setup, mag2flux
from test_gpu_rhmc_diag import WALL_MAG, _field, _rel_each

pytestmark = pytest.mark.gpu

F, XY, NONFINITE, PCAP, QCAP, NEAR = 8, 16, 1, 2, 4, 32
REF_FWHM = default_exp_setup()[3]     # the reference PSF, 3.5 px
WIDE_FWHM = 3.8     # inside (3.555, 4.06]: the 32-px one-star window by rule
STEP_BAR = (1e-11, 1e-10)       # q, p: one step from the oracle's state
FUSED_BAR = (1e-9, 1e-8)        # q, p: all steps in one launch
DELTA = 1e-6


def _steps(K):
    return 8 if K <= 64 else 3 if K <= 256 else 2 if K <= 520 else 1


def _row(K, side, n, kernel, split, fwhm, f32, body):
    return (K, side, n, kernel, split, fwhm, f32, _steps(K), body)


# id: K, image side, chains, forced kernel, RHMC_OPT_WINDOW_SPLIT, PSF FWHM,
# image exact in fp32 (else the same image + 0.1), steps, body key
TABLE = {}
# one star, register window: 5 chains are one full wave and a one-chain wave;
# 17 chains (48 px, 28-px window, fp32) a second workgroup, partly filled.  On
# 96 / 128 px the chains sit at both clamped window corners and mid-image.
for _side in (32, 48, 64, 96, 128):
    for _win, _fwhm in ((28, REF_FWHM), (32, WIDE_FWHM)):
        for _f32 in (True, False):
            _n = 17 if (_side, _win, _f32) == (48, 28, True) else 5
            TABLE["k1_regwin%d_w%d_%s" % (_side, _win, "f32" if _f32 else "f64")] = _row(
                1, _side, _n, None, 0, _fwhm, _f32,
                "regwin1/%d/%d/%s" % (_side, _win, "float" if _f32 else "double"))
# one star, lane groups: 16 lanes per chain at 5 chains (17 once), one lane
# per chain at 65 chains (a full wave and a one-chain wave); the fp64 cache
# on the image + 0.1, whose pixels an fp32 cache would round (at 32 px forced
# with lane1_f64 as well, which the plan then does not need)
for _side in (32, 48, 64):
    TABLE["k1_lane4_%d_f32" % _side] = _row(1, _side, 17 if _side == 32 else 5, "lane4", 0,
                                            REF_FWHM, True, "lane/%d/float/4" % _side)
    TABLE["k1_lane4_%d_f64" % _side] = _row(1, _side, 5, "lane4", 0, REF_FWHM, False,
                                            "lane/%d/double/4" % _side)
    TABLE["k1_lane1_%d_f32" % _side] = _row(1, _side, 65, "lane1", 0, REF_FWHM, True,
                                            "lane/%d/float/1" % _side)
    TABLE["k1_lane1_%d_f64" % _side] = _row(1, _side, 65, "lane1_f64" if _side == 32 else "lane1",
                                            0, REF_FWHM, False, "lane/%d/double/1" % _side)
TABLE.update({
    # pixel-major at its K limits; an odd chain count leaves half a pair empty
    "k2_pixmajor32": _row(2, 32, 3, None, 0, REF_FWHM, True, "pixmajor/32"),
    "k10_pixmajor32": _row(10, 32, 5, None, 0, REF_FWHM, True, "pixmajor/32"),
    "k3_pixmajor48": _row(3, 48, 5, None, 0, REF_FWHM, True, "pixmajor/48"),
    "k10_pixmajor48": _row(10, 48, 3, None, 0, REF_FWHM, True, "pixmajor/48"),
    # multi-star register window with LDS tables; 40 px is a side no other
    # register kernel serves: one star there goes to this kernel too
    "k3_multiwin_tab": _row(3, 48, 5, "multiwin", 0, REF_FWHM, True, "multiwin/float/1/tab"),
    "k3_multiwin_tab_f64": _row(3, 48, 3, None, 0, REF_FWHM, False, "multiwin/double/1/tab"),
    "k1_multiwin_tab40": _row(1, 40, 5, None, 0, REF_FWHM, True, "multiwin/float/1/tab"),
})
# without tables: one slot (K = 3, forced) and two (K = 33: slot 1 holds one
# star; K = 64: both full), each window split set with the option
for _dt, _f32 in (("float", True), ("double", False)):
    for _i, _ws in enumerate((1, 2, 4)):
        TABLE["k3_notab_%s_ws%d" % (_dt, _ws)] = _row(
            3, 48, (3, 5)[_i % 2], "multiwin_notab", _ws, REF_FWHM, _f32,
            "multiwin/%s/1/notab/%d" % (_dt, _ws))
        _K = (33, 64)[(_i + (not _f32)) % 2]
        TABLE["k%d_notab_%s_ws%d" % (_K, _dt, _ws)] = _row(
            _K, 64, (5, 3)[_i % 2], None, _ws, REF_FWHM, _f32,
            "multiwin/%s/2/notab/%d" % (_dt, _ws))
TABLE.update({
    # split 0: kr_window_split picks 4 below 4096 chain pairs
    "k40_notab_by_rule": _row(40, 64, 5, None, 0, REF_FWHM, True, "multiwin/float/2/notab/4"),
    # LDS image: forced (with the reference PSF the multi-star register window
    # serves every square side from 32 px), and by rule under the wider PSF
    "k1_generic40": _row(1, 40, 3, "generic", 0, REF_FWHM, True, "ldsimage/1"),
    "k2_generic40": _row(2, 40, 3, "generic", 0, REF_FWHM, True, "ldsimage/2"),
    "k3_generic40": _row(3, 40, 3, "generic", 0, REF_FWHM, True, "ldsimage/4"),
    "k5_generic40": _row(5, 40, 3, "generic", 0, REF_FWHM, True, "ldsimage/8"),
    "k9_generic40": _row(9, 40, 3, "generic", 0, REF_FWHM, True, "ldsimage/16"),
    "k16_generic40": _row(16, 40, 3, "generic", 0, REF_FWHM, True, "ldsimage/16"),
    "k3_generic48": _row(3, 48, 3, "generic", 0, REF_FWHM, False, "ldsimage/4"),
    "k2_wide40": _row(2, 40, 3, None, 0, WIDE_FWHM, True, "ldsimage/2"),
    # slotted: the star counts of test_gpu_traj_bodies.TABLE (a last slot nearly
    # empty, a whole slot empty, all slots full)
    "k12_dense32": _row(12, 32, 3, None, 0, REF_FWHM, True, "slotted/Dense32/1"),
    "k70_dense32": _row(70, 32, 2, None, 0, REF_FWHM, True, "slotted/Dense32/2"),
    "k256_dense32": _row(256, 32, 2, None, 0, REF_FWHM, True, "slotted/Dense32/4"),
    "k12_dense48": _row(12, 48, 3, None, 0, REF_FWHM, True, "slotted/Dense48/1"),
    "k70_dense48": _row(70, 48, 2, None, 0, REF_FWHM, True, "slotted/Dense48/2"),
    "k129_dense48": _row(129, 48, 2, None, 0, REF_FWHM, True, "slotted/Dense48/4"),
    "k70_wingg2": _row(70, 64, 2, None, 0, REF_FWHM, True, "slotted/WinGG/2"),
    "k130_wingg4": _row(130, 64, 2, None, 0, REF_FWHM, True, "slotted/WinGG/4"),
    "k260_wingg8": _row(260, 32, 2, None, 0, REF_FWHM, True, "slotted/WinGG/8"),
    "k520_wingg16": _row(520, 32, 2, None, 0, REF_FWHM, True, "slotted/WinGG/16"),
    "k1024_wingg16": _row(1024, 32, 2, None, 0, REF_FWHM, True, "slotted/WinGG/16"),
    "k12_windowed": _row(12, 32, 3, "windowed", 0, REF_FWHM, True, "slotted/WinG/1"),
    "k64_windowed": _row(64, 48, 2, "windowed", 0, REF_FWHM, True, "slotted/WinG/1"),
})
FREE_ONLY = ("k1024_wingg16",)      # one step: no room for a crossing and steps past it
WALL_ROWS = [name for name in TABLE if name not in FREE_ONLY]
# one row per family
CAP_ROWS = ["k1_regwin64_w28_f64", "k1_lane4_32_f32", "k1_lane1_48_f32", "k3_pixmajor48",
            "k3_multiwin_tab", "k33_notab_float_ws1", "k3_generic40", "k12_dense32", "k12_windowed"]
# the bodies that share a wave among chains: bit-identical mates, or within
# 1e-12 (the documented per-wave fallback of DESIGN section 8)
NAN_ROWS = {"k1_regwin64_w28_f32": 1e-12, "k1_regwin128_w32_f64": 1e-12, "k2_pixmajor32": 1e-12,
            "k10_pixmajor48": 1e-12, "k1_lane4_48_f32": 0., "k1_lane1_64_f64": 0.,
            "k3_multiwin_tab_f64": 0., "k3_notab_float_ws2": 0., "k33_notab_double_ws2": 0.}
_cache = {}


def launch_counts(name):
    """Every chain count the tests below launch for a row: all chains, the
    batch-invariance subset and the one-chain rerun, the even and the odd
    chains of `wall`."""
    n = TABLE[name][2]
    return sorted({n, len(_subset(n)), 1, (n + 1) // 2, n // 2})


def _subset(n):
    return [0, n - 1] if n > 2 else [n - 1]


class _Oracle(RefModel):
    """oracle.rhmc_ref.RefModel with dphidq scaled (1.0: the oracle's own bits)."""

    def __init__(self, D, par, scale_G=1.):
        RefModel.__init__(self, D, par)
        self.scale_G = scale_G

    def dphidq(self, q):
        return RefModel.dphidq(self, q) * self.scale_G


def _shape(name):
    """A row of TABLE by its id; a row given itself (tests/test_gpu_ragged_bodies.py
    builds its own rows' fields and oracle runs with the helpers below)."""
    return TABLE[name] if isinstance(name, str) else name


def _dt(K):
    return 0.1 if K <= 3 else 0.05 if K <= 16 else 0.02


def _par(name, prior, f_lim, cap=False):
    """rhmc_params of one run (capi.make_params' keywords)."""
    K, fwhm = _shape(name)[0], _shape(name)[5]
    par, _ = workloads.base_params(_dt(K) * (10. if cap else 1.), g_xx=0.05, g_ff=4., g_ff2=4.,
                                   use_prior=prior, alpha=2.)
    assert par["fwhm_pix"] == REF_FWHM
    par.update(fwhm_pix=fwhm, f_lim=f_lim, delta=1e-10 if cap else DELTA,
               counter_max=2 if cap else 1000)
    return par


def _model(name, D, par, scale_G=1.):
    side = _shape(name)[1]
    return _Oracle(D, dict(par, rows=side, cols=side, fmin=-1., fmax=-1.), scale_G)


def _start(name):
    """(D, q0, z) of a row.  One star on 96 / 128 px: three stars in the image,
    at both corners and mid-image, and the chains near them in turn."""
    K, side, n, _, _, _, f32, _, _ = _shape(name)
    if K == 1 and side >= 96:
        _, _, ftc, fwhm, B, _, _, _ = default_exp_setup()
        rng = np.random.RandomState(100 + side)
        stars = [(20.0, 6.3, 7.1), (20.5, side / 2. + 0.4, side / 2. - 0.3),
                 (19.8, side - 7.2, side - 6.6)]
        D = workloads._image(side, stars, ftc, B, fwhm, rng)
        q0 = np.array([[mag2flux(stars[c % 3][0]) * ftc, stars[c % 3][1], stars[c % 3][2]]
                       for c in range(n)])
        q0[:, 0] *= np.exp(0.03 * rng.randn(n))
        q0[:, 1:] += 0.2 * rng.randn(n, 2)
        z = rng.randn(n, 3)
    else:
        D, q0, z = _field(K, side, n, 100 + K + side)
    if not f32:
        D = D + 0.1
    assert np.array_equal(D, D.astype(np.float32).astype(float)) == f32
    return D, q0, z


def _run(m, q, p, n, par):
    """n oracle steps of one chain: states, counts per step, the status word,
    the least |test value / delta - 1| and the least relative distance of a
    flux or coordinate from the wall it is compared with."""
    side, f_lim, delta, cm = m.rows, par["f_lim"], par["delta"], par["counter_max"]
    Q, P, NP, NQ, ST, margin, clear = [q], [p], [], [], [], np.inf, np.inf
    for _ in range(n):
        tr, st = {}, 0
        q, p, a, b = m.step(q, p, delta, cm, trace=tr)
        Q.append(q)
        P.append(p)
        NP.append(a)
        NQ.append(b)
        if a == cm and tr["dp"][-1] > delta:
            st |= PCAP
        if b == cm and tr["dq"][-1] > delta:
            st |= QCAP
        f, x, y = q[0::3], q[1::3], q[2::3]
        if (f < f_lim).any():
            st |= F
        if ((x < 0) | (x > side - 1) | (y < 0) | (y > side - 1)).any():
            st |= XY
        v = np.array(tr["dp"] + tr["dq"])
        margin = min(margin, np.abs(v / delta - 1.).min())
        xy = np.concatenate([x, y])
        clear = min(clear, np.abs(xy).min() / (side - 1.), np.abs(xy - (side - 1.)).min() / (side - 1.),
                    np.abs(f / f_lim - 1.).min() if f_lim > 0 else np.inf)
        assert (f > 0).all()
        ST.append(st)
    return dict(Q=np.array(Q), P=np.array(P), NP=np.array(NP), NQ=np.array(NQ), ST=np.array(ST),
                st=int(np.bitwise_or.reduce(ST)) if ST else 0, margin=margin, clear=clear)


def _conditioned(name, D, par, q0, p0, n, want, bar, stepwise):
    """The three conditions on one chain's run; returns the sensitivity figure
    as a fraction of the bar (at most 0.1)."""
    assert want["margin"] > 1e-9, (name, want["margin"])
    assert want["clear"] > 1e-7, (name, want["clear"])
    worst = 0.
    for sG in (1 + 1e-13, 1 - 1e-13):
        m = _model(name, D, par, sG)
        got = _run(m, q0, p0, n, par)
        assert np.array_equal(got["NP"], want["NP"]) and np.array_equal(got["NQ"], want["NQ"]) \
            and got["st"] == want["st"], name
        worst = max(worst, _rel_each(got["Q"][-1], want["Q"][-1]) / bar[0],
                    _rel_each(got["P"][-1], want["P"][-1]) / bar[1])
        if stepwise:
            for s in range(n):
                q, p, a, b = m.step(want["Q"][s], want["P"][s], par["delta"], par["counter_max"])
                assert (a, b) == (want["NP"][s], want["NQ"][s]), (name, s)
                worst = max(worst, _rel_each(q, want["Q"][s + 1]) / STEP_BAR[0],
                            _rel_each(p, want["P"][s + 1]) / STEP_BAR[1])
    assert worst <= 0.1, (name, worst)
    return worst


def _case(name, scen, D, par, q0, p0, n_of, bar, stepwise=False):
    """Runs every chain on the oracle for its own step count and asserts the
    conditions: dict of D, par, q0, p0, the runs, the conditioning figure."""
    t0 = time.time()
    m = _model(name, D, par)
    want, cond = [], 0.
    for c in range(len(q0)):
        want.append(_run(m, q0[c], p0[c], int(n_of[c]), par))
        cond = max(cond, _conditioned(name, D, par, q0[c], p0[c], int(n_of[c]), want[c], bar,
                                      stepwise))
    return dict(D=D, par=par, q0=q0, p0=p0, n_of=np.array(n_of), want=want, cond=cond,
                margin=min(w["margin"] for w in want), clear=min(w["clear"] for w in want),
                cpu_s=time.time() - t0)


def _momenta(name, D, par, q0, z):
    m = _model(name, D, par)
    return z * np.sqrt(np.array([m.H(q) for q in q0]))


def free_case(name):
    if ("free", name) in _cache:
        return _cache[("free", name)]
    K, side, n, _, _, _, _, steps, _ = TABLE[name]
    D, q0, z = _start(name)
    par = _par(name, True, 0.)
    p0 = _momenta(name, D, par, q0, z)
    out = _case(name, "free", D, par, q0, p0, [steps] * n, FUSED_BAR, stepwise=True)
    assert all(w["st"] == 0 for w in out["want"]), name
    if K == 1 and side >= 96:       # both clamped window origins, and neither
        for c, w in enumerate(out["want"]):
            xy = w["Q"][:, 1:]
            assert ((xy < 10.).all(), ((xy > 14.) & (xy < side - 15.)).all(),
                    (xy > side - 11.).all())[c % 3], (name, c)
    _cache[("free", name)] = out
    return out


def edge_case(name):
    if ("edge", name) in _cache:
        return _cache[("edge", name)]
    K, side, n, _, _, _, _, steps, _ = TABLE[name]
    D, q0, z = _start(name)
    par = _par(name, True, 0.)
    p0 = _momenta(name, D, par, q0, z)
    m = _model(name, D, par)
    # half a pixel per step outwards: dq/dt = p / H_xx
    i, j = 3 * (K - 1) + 1, 2
    q0[0, i] = 0.3
    p0[0, i] = -0.5 / par["dt"] * m.H(q0[0])[i]
    q0[n - 1, j] = side - 1.3
    p0[n - 1, j] = 0.5 / par["dt"] * m.H(q0[n - 1])[j]
    out = _case(name, "edge", D, par, q0, p0, [steps] * n, FUSED_BAR)
    st = [w["st"] for w in out["want"]]
    assert st[0] == XY and st[n - 1] == XY and not any(st[1:n - 1]), (name, st)
    _cache[("edge", name)] = out
    return out


# momentum scales tried until the wall star first crosses on the chosen step
_SCALES = (1., 1.2, 0.85, 1.4, 0.7, 1.7, 0.55, 2.2, 3., 0.4, 0.3, 0.2, 0.14, 0.1, 0.07, 0.05,
           0.035, 0.025, 0.017, 0.012, 0.008)


def _aim(m, par, q, p, i, t, n_steps, f_lim):
    """The momentum of flux i with which its star first goes below the wall on
    step t (and no star before): True if one of _SCALES gives it; p is set."""
    for scale in _SCALES:   # free flight would cross halfway through step t
        p[i] = -scale * (q[i] - f_lim) / (par["dt"] * (t - 0.5)) * m.H(q)[i]
        r = _run(m, q, p, n_steps, par)
        below = (r["Q"][1:, 0::3] < f_lim).any(axis=1)
        if below.any() and int(np.argmax(below)) + 1 == t and r["Q"][t, i] < f_lim:
            return True
    return False


def wall_case(name):
    """The chains of a parity first cross on the same step, the latest of
    3, 2, 1 (2, 1 for the odd chains and from 65 stars) that every one of
    them can be aimed at: the even chains end there, the odd chains run
    `past` steps more."""
    if ("wall", name) in _cache:
        return _cache[("wall", name)]
    K, side, n, _, _, _, _, steps, _ = TABLE[name]
    D, q0, z = _start(name)
    f_lim = mag2flux(WALL_MAG) * default_exp_setup()[2]
    par = _par(name, False, f_lim)
    p0 = _momenta(name, D, par, q0, z)
    m = _model(name, D, par)
    star = np.where(np.arange(n) % 2 == 0, K - 1, 0)
    for c in range(n):
        q0[c, 3 * star[c]] = f_lim * (1.02 + 0.01 * (c % 8))
    past = 4 if steps >= 8 else 2
    launches, n_of = [], np.zeros(n, int)
    for parity, tries in ((0, (3, 2, 1) if steps >= 8 else (2, 1)),
                          (1, (2, 1) if steps >= 8 else (1,))):
        chains = list(range(parity, n, 2))
        for t in tries:
            n_steps = t + past * parity
            if all(_aim(m, par, q0[c], p0[c], 3 * star[c], t, n_steps, f_lim) for c in chains):
                break
        else:
            raise AssertionError((name, parity, "no common crossing step"))
        n_of[chains] = n_steps
        launches.append((chains, n_steps))
    out = _case(name, "wall", D, par, q0, p0, n_of, FUSED_BAR)
    out.update(f_lim=f_lim, star=star, launches=launches)
    assert all(w["st"] & F for w in out["want"]), (name, [w["st"] for w in out["want"]])
    for c in range(0, n, 2):        # the even chains end below the wall, on the flip
        assert out["want"][c]["Q"][-1, 3 * star[c]] < f_lim
    _cache[("wall", name)] = out
    return out


def cap_case(name):
    if ("cap", name) in _cache:
        return _cache[("cap", name)]
    n = TABLE[name][2]
    D, q0, z = _start(name)
    par = _par(name, True, 0., cap=True)
    p0 = _momenta(name, D, par, q0, z)
    out = _case(name, "cap", D, par, q0, p0, [2] * n, FUSED_BAR, stepwise=True)
    st = [w["st"] for w in out["want"]]
    assert any(s & PCAP for s in st) and any(s & QCAP for s in st), (name, st)
    _cache[("cap", name)] = out
    return out


def conditions(name):
    """Every scenario of a row on the CPU; {scenario: (conditioning as a
    fraction of the bar, least delta margin, least wall clearance)}."""
    cases = {"free": free_case(name), "edge": edge_case(name)}
    if name in WALL_ROWS:
        cases["wall"] = wall_case(name)
    if name in CAP_ROWS:
        cases["cap"] = cap_case(name)
    return {k: (c["cond"], c["margin"], c["clear"]) for k, c in cases.items()}


# ------------------------------------------------------------------- the GPU
class _Ctx:
    """A context on a case's image with the row's forced kernel and window split."""

    def __init__(self, capi, name, case):
        self.ctx = capi.Context(case["D"], kernel=TABLE[name][3] or "auto")
        self.ctx.set_option(capi.OPT_WINDOW_SPLIT, TABLE[name][4])

    def __enter__(self):
        return self.ctx

    def __exit__(self, *exc):
        self.ctx.close()
        return False


def _same(a, b):
    return all(np.array_equal(x, y) for x, y in zip(a, b))


def _errors(q, p, want_q, want_p):
    return _rel_each(q, want_q), _rel_each(p, want_p)


def _fused(capi, ctx, case, chains, n_steps, bar):
    """One launch of `chains`; counts and status exact, the state within `bar`;
    a subset and one chain alone bit-identical.  Returns (got, eq, ep)."""
    P = capi.make_params(**case["par"])
    q0, p0, want = case["q0"][chains], case["p0"][chains], [case["want"][c] for c in chains]
    got = ctx.leapfrog(P, q0, p0, n_steps, return_info=True)
    q, p, it, st = got
    assert np.array_equal(it[:, 0], [w["NP"].sum() for w in want])
    assert np.array_equal(it[:, 1], [w["NQ"].sum() for w in want])
    assert np.array_equal(st, [w["st"] for w in want]), (st, [w["st"] for w in want])
    eq, ep = _errors(q, p, np.array([w["Q"][-1] for w in want]),
                     np.array([w["P"][-1] for w in want]))
    for sub in (_subset(len(chains)), [len(chains) - 1]):
        assert _same(ctx.leapfrog(P, q0[sub], p0[sub], n_steps, return_info=True),
                     [a[sub] for a in got])
    assert eq <= bar[0] and ep <= bar[1], (eq, ep)
    return got, eq, ep


def _report(capsys, name, run, case, text):
    with capsys.disabled():
        print("\n  %s %s [%s]: %s; conditioning %.2g of the bar, delta margin %.2g, CPU %.1f s"
              % (name, run, TABLE[name][8], text, case["cond"], case["margin"], case["cpu_s"]))


@pytest.mark.parametrize("name", list(TABLE))
def test_free_stepwise_fused_split_and_batch(gpu_lib, name, capsys):
    capi = gpu_lib
    case = free_case(name)
    n, steps = len(case["q0"]), TABLE[name][7]
    Q = np.array([w["Q"] for w in case["want"]])
    Pm = np.array([w["P"] for w in case["want"]])
    NP = np.array([w["NP"] for w in case["want"]])
    NQ = np.array([w["NQ"] for w in case["want"]])
    P = capi.make_params(**case["par"])
    sq = sp = 0.
    with _Ctx(capi, name, case) as ctx:
        for s in range(steps):
            q, p, it, st = ctx.leapfrog(P, Q[:, s], Pm[:, s], 1, return_info=True)
            assert np.array_equal(it[:, 0], NP[:, s]) and np.array_equal(it[:, 1], NQ[:, s]), s
            assert not st.any()
            eq, ep = _errors(q, p, Q[:, s + 1], Pm[:, s + 1])
            sq, sp = max(sq, eq), max(sp, ep)
        got, fq, fp = _fused(capi, ctx, case, list(range(n)), steps, FUSED_BAR)
        if steps > 1:       # the same steps in two launches
            a = steps // 2
            q1, p1, it1, st1 = ctx.leapfrog(P, case["q0"], case["p0"], a, return_info=True)
            q2, p2, it2, st2 = ctx.leapfrog(P, q1, p1, steps - a, return_info=True)
            assert _same((q2, p2, it1 + it2, st1 | st2), got)
    _report(capsys, name, "free", case, "stepwise q %.2g p %.2g (bars 1e-11, 1e-10), fused q %.2g "
            "p %.2g (1e-9, 1e-8)" % (sq, sp, fq, fp))
    assert sq <= STEP_BAR[0] and sp <= STEP_BAR[1]


@pytest.mark.parametrize("name", list(TABLE))
def test_edge_reflections(gpu_lib, name, capsys):
    capi = gpu_lib
    case = edge_case(name)
    with _Ctx(capi, name, case) as ctx:
        (_, _, _, st), eq, ep = _fused(capi, ctx, case, list(range(len(case["q0"]))),
                                       TABLE[name][7], FUSED_BAR)
    assert st[0] == XY and st[-1] == XY and not (st & NEAR).any()
    _report(capsys, name, "edge", case, "q %.2g p %.2g" % (eq, ep))


@pytest.mark.parametrize("name", WALL_ROWS)
def test_flux_wall(gpu_lib, name, capsys):
    capi = gpu_lib
    case = wall_case(name)
    worst = []
    with _Ctx(capi, name, case) as ctx:
        for chains, n_steps in case["launches"]:
            (q, _, _, st), eq, ep = _fused(capi, ctx, case, chains, n_steps, FUSED_BAR)
            assert (st & F).all()
            worst.append((eq, ep))
            if chains[0] == 0:      # ended on the flip: the wall star is still below
                for k, c in enumerate(chains):
                    assert q[k, 3 * case["star"][c]] < case["f_lim"]
    _report(capsys, name, "wall", case, "even chains q %.2g p %.2g, odd q %.2g p %.2g"
            % (worst[0] + worst[1]))


@pytest.mark.parametrize("name", CAP_ROWS)
def test_loop_caps(gpu_lib, name, capsys):
    capi = gpu_lib
    case = cap_case(name)
    want = case["want"]
    P = capi.make_params(**case["par"])
    sq = sp = 0.
    with _Ctx(capi, name, case) as ctx:
        for s in range(2):      # each step from the oracle's own state, at the stepwise bar
            q, p, it, st = ctx.leapfrog(P, [w["Q"][s] for w in want], [w["P"][s] for w in want],
                                        1, return_info=True)
            assert np.array_equal(it[:, 0], [w["NP"][s] for w in want])
            assert np.array_equal(it[:, 1], [w["NQ"][s] for w in want])
            assert np.array_equal(st, [w["ST"][s] for w in want])
            eq, ep = _errors(q, p, np.array([w["Q"][s + 1] for w in want]),
                             np.array([w["P"][s + 1] for w in want]))
            sq, sp = max(sq, eq), max(sp, ep)
        _, fq, fp = _fused(capi, ctx, case, list(range(len(case["q0"]))), 2, FUSED_BAR)
    _report(capsys, name, "cap", case, "stepwise q %.2g p %.2g, both steps q %.2g p %.2g"
            % (sq, sp, fq, fp))
    assert sq <= STEP_BAR[0] and sp <= STEP_BAR[1]


@pytest.mark.parametrize("name", list(NAN_ROWS))
def test_nan_chain_beside_wave_mates(gpu_lib, name):
    """Chain 1 starts with a NaN flux: exactly the NONFINITE bit, and its
    wave-mates as without it."""
    capi = gpu_lib
    case = free_case(name)
    q0, p0, steps, tol = case["q0"], case["p0"], TABLE[name][7], NAN_ROWS[name]
    qb = q0.copy()
    qb[1, 0] = np.nan
    P = capi.make_params(**case["par"])
    with _Ctx(capi, name, case) as ctx:
        q, p, it, st = ctx.leapfrog(P, q0, p0, steps, return_info=True)
        q2, p2, it2, st2 = ctx.leapfrog(P, qb, p0, steps, return_info=True)
    assert st2[1] == NONFINITE and np.isnan(q2[1, 0])
    others = [c for c in range(len(q0)) if c != 1]
    assert np.array_equal(st2[others], st[others]) and np.array_equal(it2[others], it[others])
    if tol == 0.:
        assert np.array_equal(q2[others], q[others]) and np.array_equal(p2[others], p[others])
    else:
        assert _rel_each(q2[others], q[others]) <= tol and _rel_each(p2[others], p[others]) <= tol
