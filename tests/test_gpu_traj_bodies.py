"""Every kernel body of the random-length trajectory, for both samplers.

rhmc_diag_random (RHMC_random_diag) and rhmc_hmc_random (HMC_random) launch one
of 25 kernel bodies each (csrc/rhmc_launch.hpp: launch_hmc_random_t), all of
which run random_trajectory<SLOTS, DIAG> of csrc/rhmc_traj.hpp.  TABLE holds at
least one shape per body, with the body's key beside it;
tests/test_traj_bodies.py checks on the CPU (tests/native/traj_bodies.cpp,
which asks csrc/rhmc_select.hpp and the launchers' own
csrc/rhmc_dispatch.hpp) that every shape is served by the body written here
and that the table covers all 25.

Each shape runs `free` (no flux wall; unequal lengths inside a wave) and
`wall`.  The star sent into the wall is star K - 1 in even chains (the last
star: the highest used slot of a multi-slot body) and star 0 in odd chains;
even chains end ON their first flipped step (the start momentum comes back),
odd chains four steps past it.

* RHMC_random_diag against the NumPy restatement tests/rhmc_diag_ref.py: end
  states, status words, the stale momentum, batch invariance, the trace.
* HMC_random against oracle.rhmc_ref.RefModel.hmc_random_traj: end states,
  status words, batch invariance.
* A NaN chain beside wave-mates in the bodies that share a wave among chains.

Bars.  q and p: 1e-10 of max|value| + 1, the bar of test_gpu_rhmc_diag.py and
test_gpu_samplers.py.  It is conditional on the shape: the CPU side first
replays every chain with the gradient scaled by 1 +- 1e-13 and asserts that
the end state moves by at most a tenth of the bar and that no flip flag
changes, so the bar tests the kernels' arithmetic, not the shape's stability.
"""
import time

import numpy as np
import pytest

import rhmc_diag_ref
from oracle.rhmc_ref import RefModel
from rhmc_amd.photometry import mag2flux
from rhmc_amd.samplers import lightsource_gym
from test_gpu_rhmc_diag import BAR, WALL_MAG, WALL_STEPS, _field, _gym, _rel, _rel_each

pytestmark = pytest.mark.gpu

_L5 = (17, 1, 30, 12, 23)
_L3 = (14, 1, 9)
# id: K, image side, chains, forced kernel, step of RHMC_random_diag, trajectory
# lengths of `free`, image exact in fp32 (else the same image + 0.1), body key.
# The first nine are the shapes of test_gpu_rhmc_diag.CASES.
TABLE = {
    "k1_regwin": (1, 32, 5, None, 0.2, _L5, True, "regwin1/32/float"),
    "k1_windowed": (1, 48, 5, "windowed", 0.2, _L5, True, "slotted/WinG/1"),
    "k3_pixmajor": (3, 48, 5, None, 0.1, _L5, True, "pixmajor/48"),
    "k3_multiwin": (3, 48, 5, "multiwin", 0.1, _L5, True, "multiwin/float/1/tab"),
    "k3_multiwin_notab": (3, 48, 5, "multiwin_notab", 0.1, _L5, True, "multiwin/float/1/notab"),
    "k12_dense": (12, 32, 3, None, 0.05, _L3, True, "slotted/Dense32/1"),
    "k12_windowed": (12, 32, 3, "windowed", 0.05, _L3, True, "slotted/WinG/1"),
    "k70_two_slots": (70, 32, 2, None, 0.02, (9, 6), True, "slotted/Dense32/2"),
    "k40_multiwin_two_slots": (40, 64, 3, None, 0.02, (9, 1, 6), True, "multiwin/float/2/notab"),
    # one star: the other sides, and the fp64 pixel cache
    "k1_regwin48": (1, 48, 5, None, 0.2, _L5, True, "regwin1/48/float"),
    "k1_regwin64": (1, 64, 5, None, 0.2, _L5, True, "regwin1/64/float"),
    "k1_regwin32_f64": (1, 32, 5, None, 0.2, _L5, False, "regwin1/32/double"),
    "k1_regwin48_f64": (1, 48, 5, None, 0.2, _L5, False, "regwin1/48/double"),
    "k1_regwin64_f64": (1, 64, 5, None, 0.2, _L5, False, "regwin1/64/double"),
    # pixel-major at 32 px, at the kernel's K limits
    "k2_pixmajor32": (2, 32, 3, None, 0.1, _L3, True, "pixmajor/32"),
    "k10_pixmajor32": (10, 32, 3, None, 0.05, _L3, True, "pixmajor/32"),
    # multi-star register window on an fp64 image (pixel-major needs fp32).
    # K = 33: slot 1 holds one star, the odd chain count leaves half a wave empty
    "k3_multiwin_f64": (3, 48, 3, None, 0.1, _L3, False, "multiwin/double/1/tab"),
    "k3_multiwin_notab_f64": (3, 48, 3, "multiwin_notab", 0.1, _L3, False,
                              "multiwin/double/1/notab"),
    "k33_multiwin_f64": (33, 64, 3, None, 0.02, (9, 1, 6), False, "multiwin/double/2/notab"),
    # global tables: 130 / 260 / 520 leave the last used slot nearly empty and
    # at least one whole slot without a star; 1024 fills all sixteen
    "k70_wingg2": (70, 64, 2, None, 0.02, (9, 6), True, "slotted/WinGG/2"),
    "k130_wingg4": (130, 64, 2, None, 0.02, (9, 6), True, "slotted/WinGG/4"),
    "k260_wingg8": (260, 32, 2, None, 0.02, (9, 6), True, "slotted/WinGG/8"),
    # (shorter there: a launch takes about 0.1 s per step at 520 stars, 0.4 s at 1024)
    "k520_wingg16": (520, 32, 2, None, 0.02, (5, 3), True, "slotted/WinGG/16"),
    "k1024_wingg16": (1024, 32, 2, None, 0.02, (2, 1), True, "slotted/WinGG/16"),
    # dense: 48 px at every slot count, four slots at 32 px (256 fills them)
    "k12_dense48": (12, 48, 3, None, 0.05, _L3, True, "slotted/Dense48/1"),
    "k70_dense48": (70, 48, 2, None, 0.02, (9, 6), True, "slotted/Dense48/2"),
    "k129_dense48": (129, 48, 2, None, 0.02, (9, 6), True, "slotted/Dense48/4"),
    "k256_dense32": (256, 32, 2, None, 0.02, (9, 6), True, "slotted/Dense32/4"),
}
FREE_ONLY = ("k1024_wingg16",)      # the wall look-ahead costs 50 s of NumPy there
RUNS = [(name, wall) for name in TABLE for wall in (False, True)
        if not (wall and name in FREE_ONLY)]
RUN_IDS = ["%s-%s" % (name, "wall" if wall else "free") for name, wall in RUNS]

# From this many stars the wall cases look 12 steps ahead, not WALL_STEPS, with
# a harder kick (z = -6 instead of -2): the restatement costs K x pixels per
# gradient, and the first crossing then comes at step 2.
SHORT_FROM_K = 129
SHORT_STEPS = 12
# HMC_random's step per star (flux, x, y), and the step count that sets the
# wall star's start momentum (hmc_case; the first crossing comes at step 2)
HMC_DT = (1.0, 0.005, 0.005)
HMC_WALL_IN = 3.5
_cache = {}


def _start(name, wall):
    """(D, q0, z, f_lim, the wall star of every chain) of one run."""
    K, side, n, _, _, _, f32, _ = TABLE[name]
    D, q0, z = _field(K, side, n, 100 + K + side)
    if not f32:
        D = D + 0.1
    assert np.array_equal(D, D.astype(np.float32).astype(float)) == f32
    star = np.where(np.arange(n) % 2 == 0, K - 1, 0)
    f_lim = 0.
    if wall:
        f_lim = mag2flux(WALL_MAG) * lightsource_gym().flux_to_count
        for c in range(n):
            q0[c, 3 * star[c]] = f_lim * (1.02 + 0.01 * c)
    return D, q0, z, f_lim, star


def _wall_steps(trace_of, n, f_lim, star, look):
    """Trajectories do not depend on their length: look `look` steps ahead, end
    even chains ON their first flipped step and odd ones four steps past it.
    The first star below the wall is the chain's wall star, and no decision
    falls on the edge."""
    steps = np.zeros(n, np.int32)
    for c in range(n):
        tr = trace_of(c, look)
        below = (tr[1:, 0::3] < f_lim).any(axis=1)
        assert below.any(), c
        first = int(np.argmax(below)) + 1
        assert tr[first, 3 * star[c]] < f_lim, c
        steps[c] = first if c % 2 == 0 else min(first + 4, look)
        f = tr[:steps[c] + 1, 0::3]
        assert (np.abs(f - f_lim) > 1e-7 * f_lim).all(), c
    return steps


def _sensitivity(replay, want):
    """The chain's end state under a gradient scaled by 1 +- 1e-13 stays within
    a tenth of the bar and flips where the unscaled one does (the condition of
    test_gpu_rhmc_diag._conditioned); returns the figure."""
    worst = 0.
    for sG in (1 + 1e-13, 1 - 1e-13):
        got = replay(sG)
        assert got[2] == want[2]
        worst = max(worst, _rel(got[0], want[0]), _rel(got[1], want[1]))
    assert worst <= 0.1 * BAR, worst
    return worst


def diag_case(name, wall):
    """RHMC_random_diag's run: dict of D, f_lim, q0, p0, steps, the restatement's
    (q, p, flipped, trace) per chain, the conditioning figure, CPU seconds."""
    if ("diag", name, wall) in _cache:
        return _cache[("diag", name, wall)]
    t0 = time.time()
    K, side, n, _, dt, steps, _, _ = TABLE[name]
    D, q0, z, f_lim, star = _start(name, wall)
    short = K >= SHORT_FROM_K
    if wall:
        for c in range(n):
            z[c, 3 * star[c]] = (-6.0 if short else -2.0) - 0.1 * c
    g = lightsource_gym()
    g.num_rows = g.num_cols = side
    g.compute_factors()
    r_args = (D, g.B_count, g.PSF_FWHM_pix, g.factor1)
    r = rhmc_diag_ref.DiagRef(*r_args)
    p0 = z * np.sqrt(np.array([r.mass_matrix(q) for q in q0]))
    steps = np.array(steps, np.int32)
    if wall:
        steps = _wall_steps(lambda c, m: r.traj(q0[c], p0[c], m, dt, f_lim)[3], n, f_lim, star,
                            SHORT_STEPS if short else WALL_STEPS)
    want = [r.traj(q0[c], p0[c], int(steps[c]), dt, f_lim) for c in range(n)]
    cond = max(_sensitivity(lambda sG: rhmc_diag_ref.DiagRef(*r_args, scale_G=sG).traj(
        q0[c], p0[c], int(steps[c]), dt, f_lim), want[c]) for c in range(n))
    out = dict(D=D, f_lim=f_lim, q0=q0, p0=p0, steps=steps, dt=dt, want=want, cond=cond,
               cpu_s=time.time() - t0)
    _cache[("diag", name, wall)] = out
    return out


class _Oracle(RefModel):
    """oracle.rhmc_ref.RefModel with the gradient scaled (1.0: the oracle's own
    bits) and every point at which hmc_random_traj asks for it kept: the start,
    then q after each step (and the end once more)."""

    def __init__(self, D, par, scale_G=1.):
        RefModel.__init__(self, D, par)
        self.scale_G = scale_G
        self.seen = []

    def dVdq(self, q):
        self.seen.append(np.array(q))
        return RefModel.dVdq(self, q) * self.scale_G

    def trace(self, q, p, dt, steps, f_lim):
        self.seen = []
        self.hmc_random_traj(q, p, dt, steps, f_lim)
        return np.array(self.seen[:steps + 1])


def hmc_case(name, wall):
    """HMC_random's run on the same image and starts: unit-mass momenta, the
    step vector HMC_DT per star."""
    if ("hmc", name, wall) in _cache:
        return _cache[("hmc", name, wall)]
    t0 = time.time()
    K, side, n, _, _, steps, _, _ = TABLE[name]
    D, q0, p0, f_lim, star = _start(name, wall)
    dt = np.tile(HMC_DT, K)
    g = lightsource_gym()
    par = dict(rows=side, cols=side, B_count=g.B_count, fwhm_pix=g.PSF_FWHM_pix, use_prior=0,
               use_Vc=0, alpha=2., beta=1., Vc_r_pow=1., dt=1., f_lim=f_lim, f_low=1., g_xx=1.,
               g_ff=1., g_ff2=1., g0=1., g1=1., g2=1., fmin=-1., fmax=-1.)
    m = _Oracle(D, par)
    if wall:        # the wall star, started well below its true flux, is pushed up: the
        # momentum that takes it in s = HMC_WALL_IN steps as far below the wall as it starts
        # above, were that push constant: f_lim - (f - f_lim) = f + dt s p - dt^2 s^2 dVdf / 2
        for c in range(n):
            i, s = 3 * star[c], HMC_WALL_IN
            p0[c, i] = (2 * (f_lim - q0[c, i]) + (dt[i] * s) ** 2 * m.dVdq(q0[c])[i] / 2.) \
                / (dt[i] * s)
    steps = np.array(steps, np.int32)
    if wall:
        steps = _wall_steps(lambda c, k: m.trace(q0[c], p0[c], dt, k, f_lim), n, f_lim, star,
                            SHORT_STEPS)
    want, mid = [], 0       # mid: chains with a step below the wall before their last
    for c in range(n):
        m.seen = []
        want.append(m.hmc_random_traj(q0[c], p0[c], dt, int(steps[c]), f_lim))
        mid += bool((np.array(m.seen[1:steps[c]])[:, 0::3] < f_lim).any()) if steps[c] > 1 else 0
    cond = max(_sensitivity(lambda sG: _Oracle(D, par, sG).hmc_random_traj(
        q0[c], p0[c], dt, int(steps[c]), f_lim), want[c]) for c in range(n))
    out = dict(D=D, f_lim=f_lim, q0=q0, p0=p0, steps=steps, dt=dt, want=want, cond=cond,
               mid=mid, cpu_s=time.time() - t0)
    _cache[("hmc", name, wall)] = out
    return out


class _Gym:
    """The sampler object on a case's image, with the forced kernel; closes its
    context on the way out."""

    def __init__(self, name, case):
        self.g = _gym(case["D"], case["f_lim"])
        self.kernel = TABLE[name][3] or "auto"

    def __enter__(self):
        ctx = self.g._context()
        ctx.set_kernel(self.kernel)
        return self.g, ctx

    def __exit__(self, *exc):
        self.g._context().close()
        return False


def _subset(n):
    return [0, n - 1] if n > 2 else [n - 1]


def _assert_run_shape(case, wall, flipped, mid):
    steps, n = case["steps"], len(case["q0"])
    if wall:        # some chain ends on a flip, some chain flips before its end
        assert flipped.sum() > 0 and mid > 0
        assert flipped[0::2].all()
    else:           # unequal lengths inside a wave; a one-step chain wherever there are three
        assert len(set(steps)) == n and (n < 3 or steps.min() == 1)


@pytest.mark.parametrize("name,wall", RUNS, ids=RUN_IDS)
def test_diag_trajectories_status_batch_and_trace(gpu_lib, name, wall, capsys):
    capi = gpu_lib
    case = diag_case(name, wall)
    q0, p0, steps, dt, want = (case[k] for k in ("q0", "p0", "steps", "dt", "want"))
    n = len(q0)
    with _Gym(name, case) as (g, ctx):
        P = g._params()
        q, p, st = ctx.diag_random(P, dt, g.factor1, q0, p0, steps, return_status=True)
        sub = _subset(n)
        qs, ps, sts = ctx.diag_random(P, dt, g.factor1, q0[sub], p0[sub], steps[sub],
                                      return_status=True)
        qt, pt, tr = ctx.diag_random(P, dt, g.factor1, q0, p0, steps, trace=True)
    worst = 0.
    for c in range(n):
        worst = max(worst, _rel(q[c], want[c][0]), _rel(p[c], want[c][1]))
    with capsys.disabled():
        print("\n  diag %s %s [%s]: worst %.3g of max|value| + 1 (bar 1e-10), conditioning %.3g, "
              "CPU %.1f s" % (name, "wall" if wall else "free", TABLE[name][7], worst,
                              case["cond"], case["cpu_s"]))
    assert worst <= BAR
    flipped = np.array([w[2] for w in want])
    assert np.array_equal(st, np.where(flipped, capi.STATUS_REFLECT_F, 0))
    assert np.array_equal(p[flipped], p0[flipped])              # the stale momentum
    _assert_run_shape(case, wall, flipped,
                      sum(bool((w[3][1:-1, 0::3] < case["f_lim"]).any()) for w in want))
    # batch invariance: a subset gives the same bits
    assert np.array_equal(qs, q[sub]) and np.array_equal(ps, p[sub], equal_nan=True)
    assert np.array_equal(sts, st[sub])
    # the trace: rows 0 .. steps[c], the rest untouched; the results unchanged
    assert np.array_equal(qt, q) and np.array_equal(pt, p)
    assert tr.shape == (n, steps.max() + 1, q0.shape[1])
    for c in range(n):
        assert np.array_equal(tr[c, 0], q0[c])
        assert _rel(tr[c, :steps[c] + 1], want[c][3]) <= BAR
        assert np.array_equal(tr[c, steps[c]], q[c])
        assert np.isnan(tr[c, steps[c] + 1:]).all()


@pytest.mark.parametrize("name,wall", RUNS, ids=RUN_IDS)
def test_hmc_random_trajectories_status_and_batch(gpu_lib, name, wall, capsys):
    capi = gpu_lib
    case = hmc_case(name, wall)
    q0, p0, steps, dt, want = (case[k] for k in ("q0", "p0", "steps", "dt", "want"))
    n = len(q0)
    with _Gym(name, case) as (g, ctx):
        P = g._params()
        q, p, st = ctx.hmc_random(P, dt, q0, p0, steps, return_status=True)
        sub = _subset(n)
        qs, ps, sts = ctx.hmc_random(P, dt, q0[sub], p0[sub], steps[sub], return_status=True)
    worst = 0.
    for c in range(n):
        worst = max(worst, _rel(q[c], want[c][0]), _rel(p[c], want[c][1]))
    with capsys.disabled():
        print("\n  hmc %s %s [%s]: worst %.3g of max|value| + 1 (bar 1e-10), conditioning %.3g, "
              "CPU %.1f s" % (name, "wall" if wall else "free", TABLE[name][7], worst,
                              case["cond"], case["cpu_s"]))
    assert worst <= BAR
    flipped = np.array([w[2] for w in want])
    assert np.array_equal(st, np.where(flipped, capi.STATUS_REFLECT_F, 0))
    assert np.array_equal(p[flipped], p0[flipped])              # the stale momentum
    _assert_run_shape(case, wall, flipped, case["mid"])
    assert np.array_equal(qs, q[sub]) and np.array_equal(ps, p[sub])
    assert np.array_equal(sts, st[sub])


# The bodies that share a wave among chains and that test_gpu_rhmc_diag.py's
# NaN test does not run (slotted bodies have one chain per wave)
@pytest.mark.parametrize("name", ["k1_regwin64", "k3_multiwin_f64", "k33_multiwin_f64",
                                  "k2_pixmajor32"])
def test_nan_chain_beside_wave_mates(gpu_lib, name):
    """Chain 1 (the wave-mate of chain 0, and of 2 and 3 for one star) starts
    with a NaN flux: exactly the NONFINITE bit, and nobody else moves by more
    than the last bits."""
    capi = gpu_lib
    case = diag_case(name, False)
    q0, p0, steps, dt = (case[k] for k in ("q0", "p0", "steps", "dt"))
    qb = q0.copy()
    qb[1, 0] = np.nan
    with _Gym(name, case) as (g, ctx):
        P = g._params()
        q, p, st = ctx.diag_random(P, dt, g.factor1, q0, p0, steps, return_status=True)
        q2, p2, st2 = ctx.diag_random(P, dt, g.factor1, qb, p0, steps, return_status=True)
    assert st2[1] == capi.STATUS_NONFINITE
    assert np.isnan(q2[1, 0])
    others = [c for c in range(len(q0)) if c != 1]
    assert np.array_equal(st2[others], st[others])
    for c in others:
        assert _rel_each(q2[c], q[c]) <= 1e-12 and _rel_each(p2[c], p[c]) <= 1e-12
