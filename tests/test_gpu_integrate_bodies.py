"""Every kernel body of the explicit integrators, for all three solvers.

rhmc_integrate with RHMC_SOLVER_HMC, _RHMC_NAIVE or _RHMC_LEAPFROG launches one
of 25 kernel bodies (csrc/rhmc_launch.hpp: launch_integrate), each built once
per solver, around one integrator loop (explicit_steps, csrc/rhmc_traj.hpp)
and three adapters that supply the gradient, the metric and the star table:
integrate_k1_tiledr (one star), km_explicit_steps (multi-star register window
and pixel-major) and integrate_win_kernel (windowed and dense).  TABLE takes
the shapes of test_gpu_traj_bodies.TABLE, at least one per body with the body's
key beside it, and adds a step size and a step count per row;
tests/test_integrate_bodies.py checks on the CPU (tests/native/traj_bodies.cpp
in its `integrate` mode, which asks csrc/rhmc_select.hpp and the launchers' own
csrc/rhmc_dispatch.hpp) that every shape is served by the body written here and
that the table covers all 25.

Each (row, solver) runs, against oracle.rhmc_ref.RefModel's hmc_step /
rhmc_naive_step / rhmc_leapfrog_step stepped in Python:

* `free`: the flux prior on, f_pos with the wall at 0 (nothing flips), at the
  row's step count, at one step and at none (bit-identical, status 0).
* `wall`: no prior, f_pos with the wall at WALL_MAG.  The star sent into the
  wall is star K - 1 in even chains (the last star: the highest used slot of a
  multi-slot body) and star 0 in odd chains.  One launch ends the even chains
  ON their first step below the wall, a second ends the odd chains four steps
  past theirs; a third runs all chains with f_pos off (no flip, status 0).
  Unit-metric HMC has no wall: it runs the same start with f_pos on, its wall
  star sent below the wall in every chain, and must return status 0.
* A NaN chain beside wave-mates in the bodies that share a wave among chains.

Every launch: q and p per element, |got - want| / (|want| + 1) <= 1e-10 (BAR of
test_gpu_rhmc_diag.py, on the stricter per-element metric: a position beside a
1e4-count flux does not hide behind it); the status word exactly
STATUS_REFLECT_F where the oracle flipped at any step and 0 elsewhere; a subset
of the launch's chains bit-identical.  The bar is conditional on the shape: the
CPU side first replays every chain with dVdq scaled by 1 +- 1e-13 and asserts
that the end state moves by at most a tenth of the bar on the same metric and
that the same steps flip, so the bar tests the kernels' arithmetic, not the
shape's stability.  Measured on an MI355X: every body within 2.9e-13 (the worst:
multiwin/float/1, K = 3 on 48 px, naive, `free`, where the conditioning figure
is also the largest, 4.7e-12); no body takes a looser bar.
"""
import time

import numpy as np
import pytest

import test_gpu_traj_bodies as T
from rhmc_amd import workloads
from test_gpu_rhmc_diag import BAR, WALL_STEPS, _rel_each
from test_gpu_traj_bodies import SHORT_FROM_K, SHORT_STEPS, _Oracle, _start, _subset

pytestmark = pytest.mark.gpu

SOLVERS = ("hmc", "naive", "leap_frog")
# id: step of the two RHMC solvers, step of unit-metric HMC (test_gpu_integrators.
# _case: at RHMC's step its leapfrog is past the stability limit), steps of `free`
_STEPS = {
    "k1_regwin": (0.1, 0.05, 30),
    "k1_windowed": (0.1, 0.05, 30),
    "k3_pixmajor": (0.1, 0.02, 30),
    "k3_multiwin": (0.1, 0.02, 30),
    "k3_multiwin_notab": (0.1, 0.02, 30),
    "k12_dense": (0.05, 0.02, 14),
    "k12_windowed": (0.05, 0.02, 14),
    "k70_two_slots": (0.05, 0.02, 9),
    "k40_multiwin_two_slots": (0.05, 0.02, 9),
    "k1_regwin48": (0.1, 0.05, 30),
    "k1_regwin64": (0.1, 0.05, 30),
    "k1_regwin32_f64": (0.1, 0.05, 30),
    "k1_regwin48_f64": (0.1, 0.05, 30),
    "k1_regwin64_f64": (0.1, 0.05, 30),
    "k2_pixmajor32": (0.1, 0.02, 30),
    "k10_pixmajor32": (0.05, 0.02, 14),
    "k3_multiwin_f64": (0.1, 0.02, 30),
    "k3_multiwin_notab_f64": (0.1, 0.02, 30),
    "k33_multiwin_f64": (0.05, 0.02, 9),
    "k70_wingg2": (0.05, 0.02, 9),
    "k130_wingg4": (0.05, 0.02, 9),
    "k260_wingg8": (0.05, 0.02, 5),
    "k520_wingg16": (0.05, 0.02, 5),
    "k1024_wingg16": (0.05, 0.02, 2),
    "k12_dense48": (0.05, 0.02, 14),
    "k70_dense48": (0.05, 0.02, 9),
    "k129_dense48": (0.05, 0.02, 9),
    "k256_dense32": (0.05, 0.02, 5),
}
assert list(_STEPS) == list(T.TABLE)
# id: K, image side, chains, forced kernel, image exact in fp32 (else the same
# image + 0.1), body key -- the columns of test_gpu_traj_bodies.TABLE -- then
# the RHMC step, the HMC step and the step count of `free`
TABLE = {name: row[:4] + row[6:8] + _STEPS[name] for name, row in T.TABLE.items()}
FREE_ONLY = T.FREE_ONLY             # the wall look-ahead costs a minute of NumPy there
WALL_ROWS = [name for name in TABLE if name not in FREE_ONLY]
# The wall star's start momentum, in units of its own sigma, per chain c:
# _KICK - 0.1 c.  (The look-ahead of the rows from SHORT_FROM_K stars is
# SHORT_STEPS steps, not WALL_STEPS: the oracle costs K x pixels per gradient.)
_KICK = -2.0
# The start offsets tried, as multiples of the chain's own 0.02 + 0.01 c, until
# the chains of one launch first cross the wall on the same step
_OFFSETS = (1., 0.85, 1.15, 0.7, 1.3, 0.55, 1.45, 0.4, 1.6, 0.25, 1.8, 2., 2.5, 3., 4., 0.1)
_cache = {}


def _dt(name, solver):
    return TABLE[name][7 if solver == "hmc" else 6]


def _par(name, solver, use_prior, f_lim):
    """rhmc_params of one run (capi.make_params' keywords)."""
    par, _ = workloads.base_params(_dt(name, solver), g_xx=0.05, g_ff=4., g_ff2=4.,
                                   use_prior=use_prior, alpha=2.)
    par["f_lim"] = f_lim
    return par


def _model(name, D, par, scale_G=1.):
    side = TABLE[name][1]
    return _Oracle(D, dict(par, rows=side, cols=side, fmin=-1., fmax=-1.), scale_G)


def _step(m, solver, q, p, f_pos):
    m.seen = []
    if solver == "hmc":
        return m.hmc_step(q, p)
    if solver == "naive":
        return m.rhmc_naive_step(q, p, f_pos)
    return m.rhmc_leapfrog_step(q, p, f_pos)


def _flips(m, solver, q, f_pos):
    """Whether the step that ended at q flipped a momentum (the oracle's own test)."""
    return bool(f_pos and solver != "hmc" and (q[0::3] < m.p["f_lim"]).any())


def _evolve(m, solver, q, p, n, f_pos):
    """n steps: (q, p, the steps that flipped, q after every step [n + 1, 3K])."""
    flips, Q = [], [q]
    for s in range(1, n + 1):
        q, p = _step(m, solver, q, p, f_pos)
        Q.append(q)
        if _flips(m, solver, q, f_pos):
            flips.append(s)
    return q, p, tuple(flips), np.array(Q)


def _momenta(m, solver, q0, z):
    if solver == "hmc":
        return z.copy()
    return z * np.sqrt(np.array([m.H(q) for q in q0]))


def _sensitivity(name, D, par, solver, q0, p0, n, f_pos, want):
    """The chain's end state under dVdq scaled by 1 +- 1e-13 stays within a tenth
    of the bar, per element, and the same steps flip; returns the figure."""
    worst = 0.
    for sG in (1 + 1e-13, 1 - 1e-13):
        q, p, flips, _ = _evolve(_model(name, D, par, sG), solver, q0, p0, n, f_pos)
        assert flips == want[2], (name, solver, flips, want[2])
        worst = max(worst, _rel_each(q, want[0]), _rel_each(p, want[1]))
    assert worst <= 0.1 * BAR, (name, solver, worst)
    return worst


def free_case(name, solver):
    """The `free` run: dict of D, par, q0, p0, the oracle's (q, p, flips) per
    chain after n_steps (`want`) and after one step (`want1`), the
    conditioning figure, CPU seconds."""
    key = ("free", name, solver)
    if key in _cache:
        return _cache[key]
    t0 = time.time()
    n_steps = TABLE[name][8]
    D, q0, z, f_lim, _ = _start(name, False)
    assert f_lim == 0.
    par = _par(name, solver, True, f_lim)
    m = _model(name, D, par)
    p0 = _momenta(m, solver, q0, z)
    want, want1, cond = [], [], 0.
    for c in range(len(q0)):
        q, p, flips, Q = _evolve(m, solver, q0[c], p0[c], n_steps, True)
        assert flips == () and (Q[:, 0::3] > 0.).all(), (name, solver, c)
        want.append((q, p, flips))
        want1.append(_evolve(m, solver, q0[c], p0[c], 1, True)[:3])
        cond = max(cond, _sensitivity(name, D, par, solver, q0[c], p0[c], n_steps, True, want[c]),
                   _sensitivity(name, D, par, solver, q0[c], p0[c], 1, True, want1[c]))
    out = dict(D=D, par=par, q0=q0, p0=p0, n_steps=n_steps, want=want, want1=want1, cond=cond,
               cpu_s=time.time() - t0)
    _cache[key] = out
    return out


def _look(m, solver, q, p, f_lim, look, past):
    """Steps until the first flux below the wall and `past` more, `look` at the
    most: (its step or None, q after every step taken, the end as _evolve
    gives it: q, p, the steps that flipped)."""
    first, Q, flips = None, [q], []
    for s in range(1, look + 1):
        q, p = _step(m, solver, q, p, True)
        Q.append(q)
        if _flips(m, solver, q, True):
            flips.append(s)
        if first is None and (q[0::3] < f_lim).any():
            first = s
        if first is not None and s >= first + past:
            break
    return first, np.array(Q), (q, p, tuple(flips))


def wall_case(name, solver):
    """The `wall` run of an RHMC solver: dict of D, par, q0, p0, the launches
    [(chains, n_steps)] (even chains ending ON their first step below the
    wall, odd chains four steps past it), the oracle's (q, p, flips) per chain
    with f_pos (`want`) and without it at the odd chains' length (`want_off`,
    n_off), the conditioning figure, CPU seconds."""
    key = ("wall", name, solver)
    if key in _cache:
        return _cache[key]
    assert solver != "hmc"
    t0 = time.time()
    K, n = TABLE[name][0], TABLE[name][2]
    D, q0, z, f_lim, star = _start(name, True)
    look = SHORT_STEPS if K >= SHORT_FROM_K else WALL_STEPS
    par = _par(name, solver, False, f_lim)
    m = _model(name, D, par)
    for c in range(n):
        z[c, 3 * star[c]] = _KICK - 0.1 * c
    p0 = np.zeros_like(q0)
    launches, want = [], [None] * n
    for parity in (0, 1):
        steps = None
        for c in range(parity, n, 2):
            i, past = 3 * star[c], 4 * parity
            for scale in _OFFSETS:      # the first is the chain's own start, 1.02 + 0.01 c
                q0[c, i] = f_lim * (1. + scale * (0.02 + 0.01 * c))
                p0[c] = _momenta(m, solver, q0[c:c + 1], z[c:c + 1])[0]
                first, Q, want[c] = _look(m, solver, q0[c], p0[c], f_lim, look, past)
                if first is not None and first + past <= look and steps in (None, first + past):
                    break
            # every chain crosses, on the step its launch ends on or four before it;
            # the first star below the wall is the chain's wall star; no decision on the edge
            assert first is not None and first + past <= look, (name, solver, c)
            assert steps in (None, first + past), (name, solver, c, steps, first)
            steps = first + past
            assert Q[first, i] < f_lim and len(Q) == steps + 1, (name, solver, c)
            assert (np.abs(Q[:, 0::3] - f_lim) > 1e-7 * f_lim).all(), (name, solver, c)
        if steps is not None:
            launches.append((list(range(parity, n, 2)), steps))
    assert len(launches) == 2
    n_of = np.zeros(n, int)
    for chains, steps in launches:
        n_of[chains] = steps
    n_off = launches[1][1]
    want_off, cond = [], 0.
    for c in range(n):
        first = want[c][2][0]
        assert first == (n_of[c] if c % 2 == 0 else n_of[c] - 4), (name, solver, c, want[c][2])
        assert want[c][0][3 * star[c]] < f_lim or c % 2
        want_off.append(_evolve(m, solver, q0[c], p0[c], n_off, False)[:3])
        assert want_off[c][2] == ()
        cond = max(cond,
                   _sensitivity(name, D, par, solver, q0[c], p0[c], int(n_of[c]), True, want[c]),
                   _sensitivity(name, D, par, solver, q0[c], p0[c], n_off, False, want_off[c]))
    out = dict(D=D, par=par, f_lim=f_lim, star=star, q0=q0, p0=p0, launches=launches, want=want,
               want_off=want_off, n_off=n_off, cond=cond, cpu_s=time.time() - t0)
    _cache[key] = out
    return out


def hmc_wall_case(name):
    """Unit-metric HMC on the wall start (the chains' own offsets 1.02 + 0.01 c),
    the row's step count: the oracle has no wall for it.  Its momenta are not
    scaled by the metric, so _KICK would not bring the wall star down in so few
    steps: it gets the momentum that carries it, were it free, as far below the
    wall as it starts above, and every chain ends below the wall."""
    key = ("wall", name, "hmc")
    if key in _cache:
        return _cache[key]
    t0 = time.time()
    n, n_steps = TABLE[name][2], TABLE[name][8]
    D, q0, z, f_lim, star = _start(name, True)
    par = _par(name, "hmc", False, f_lim)
    m = _model(name, D, par)
    for c in range(n):
        i = 3 * star[c]
        z[c, i] = -2. * (q0[c, i] - f_lim) / (par["dt"] * n_steps)
    want, cond, below = [], 0., 0
    for c in range(n):
        q, p, flips, Q = _evolve(m, "hmc", q0[c], z[c], n_steps, True)
        want.append((q, p, flips))
        assert q[3 * star[c]] < f_lim and (np.abs(Q[:, 0::3] - f_lim) > 1e-7 * f_lim).all()
        below += bool((Q[:, 0::3] < f_lim).any())
        cond = max(cond, _sensitivity(name, D, par, "hmc", q0[c], z[c], n_steps, True, want[c]))
    assert below == n
    out = dict(D=D, par=par, f_lim=f_lim, q0=q0, p0=z, n_steps=n_steps, want=want, cond=cond,
               below=below, cpu_s=time.time() - t0)
    _cache[key] = out
    return out


def _sid(capi, solver):
    return {"hmc": capi.SOLVER_HMC, "naive": capi.SOLVER_RHMC_NAIVE,
            "leap_frog": capi.SOLVER_RHMC_LEAPFROG}[solver]


class _Ctx:
    """A context on a case's image, with the row's forced kernel."""

    def __init__(self, capi, name, case):
        self.ctx = capi.Context(case["D"], kernel=TABLE[name][3] or "auto")

    def __enter__(self):
        return self.ctx

    def __exit__(self, *exc):
        self.ctx.close()
        return False


def _launch(capi, ctx, case, solver, chains, n_steps, f_pos, want):
    """One launch of `chains`, and a subset of them on its own: asserts the
    status words (REFLECT_F exactly where the oracle flipped) and the subset's
    bits; returns (q, p, the worst per-element error against the oracle)."""
    P = capi.make_params(**case["par"])
    q0, p0 = case["q0"][chains], case["p0"][chains]
    q, p, st = ctx.integrate(P, _sid(capi, solver), q0, p0, n_steps, f_pos=f_pos,
                             return_status=True)
    sub = _subset(len(chains))
    qs, ps, sts = ctx.integrate(P, _sid(capi, solver), q0[sub], p0[sub], n_steps, f_pos=f_pos,
                                return_status=True)
    flipped = np.array([bool(want[c][2]) for c in chains])
    assert np.array_equal(st, np.where(flipped, capi.STATUS_REFLECT_F, 0)), (st, flipped)
    assert np.array_equal(qs, q[sub]) and np.array_equal(ps, p[sub]) \
        and np.array_equal(sts, st[sub])
    worst = 0.
    for k, c in enumerate(chains):
        worst = max(worst, _rel_each(q[k], want[c][0]), _rel_each(p[k], want[c][1]))
    return q, p, worst


def _report(capsys, name, run, solver, worst, case, note=""):
    with capsys.disabled():
        print("\n  %s %s %s [%s]: worst %.3g per element (bar 1e-10), conditioning %.3g, "
              "CPU %.1f s%s" % (name, run, solver, TABLE[name][5], worst, case["cond"],
                                case["cpu_s"], note))


@pytest.mark.parametrize("solver", SOLVERS)
@pytest.mark.parametrize("name", list(TABLE))
def test_free_against_the_oracle(gpu_lib, name, solver, capsys):
    capi = gpu_lib
    case = free_case(name, solver)
    everyone = list(range(len(case["q0"])))
    with _Ctx(capi, name, case) as ctx:
        _, _, worst = _launch(capi, ctx, case, solver, everyone, case["n_steps"], True,
                              case["want"])
        _, _, worst1 = _launch(capi, ctx, case, solver, everyone, 1, True, case["want1"])
        q, p, st = ctx.integrate(capi.make_params(**case["par"]), _sid(capi, solver), case["q0"],
                                 case["p0"], 0, f_pos=True, return_status=True)
    _report(capsys, name, "free", solver, max(worst, worst1), case,
            " (%d steps %.3g, one step %.3g)" % (case["n_steps"], worst, worst1))
    assert worst <= BAR and worst1 <= BAR
    # no step: nothing moves
    assert np.array_equal(q, case["q0"]) and np.array_equal(p, case["p0"]) and not st.any()


@pytest.mark.parametrize("solver", SOLVERS[1:])
@pytest.mark.parametrize("name", WALL_ROWS)
def test_wall_against_the_oracle(gpu_lib, name, solver, capsys):
    capi = gpu_lib
    case = wall_case(name, solver)
    n, f_lim, star = len(case["q0"]), case["f_lim"], case["star"]
    (even, n_even), (odd, n_odd) = case["launches"]
    assert even == list(range(0, n, 2)) and odd == list(range(1, n, 2))
    with _Ctx(capi, name, case) as ctx:
        q, _, worst_even = _launch(capi, ctx, case, solver, even, n_even, True, case["want"])
        _, _, worst_odd = _launch(capi, ctx, case, solver, odd, n_odd, True, case["want"])
        _, _, worst_off = _launch(capi, ctx, case, solver, list(range(n)), case["n_off"], False,
                                  case["want_off"])
    _report(capsys, name, "wall", solver, max(worst_even, worst_odd, worst_off), case,
            " (even chains, %d steps, %.3g; odd, %d steps, %.3g; f_pos off %.3g)" % (
                n_even, worst_even, n_odd, worst_odd, worst_off))
    assert max(worst_even, worst_odd, worst_off) <= BAR
    # the even chains ended on the flip: their wall star came back below the wall
    for k, c in enumerate(even):
        assert q[k, 3 * star[c]] < f_lim
    # some odd chain flipped before its last step (_launch has compared the status words)
    assert any(w[2] and w[2][0] < n_odd for w in (case["want"][c] for c in odd))


@pytest.mark.parametrize("name", WALL_ROWS)
def test_hmc_has_no_wall(gpu_lib, name, capsys):
    """Unit-metric HMC on the wall start with f_pos on: the oracle's plain
    leapfrog, status 0 (_launch expects REFLECT_F nowhere: hmc never flips)."""
    capi = gpu_lib
    case = hmc_wall_case(name)
    with _Ctx(capi, name, case) as ctx:
        _, _, worst = _launch(capi, ctx, case, "hmc", list(range(len(case["q0"]))),
                              case["n_steps"], True, case["want"])
    _report(capsys, name, "wall", "hmc", worst, case,
            " (%d chains with a flux below the wall)" % case["below"])
    assert worst <= BAR


# The bodies that share a wave among chains
@pytest.mark.parametrize("solver", SOLVERS)
@pytest.mark.parametrize("name", ["k1_regwin64", "k3_multiwin_f64", "k33_multiwin_f64",
                                  "k2_pixmajor32"])
def test_nan_chain_beside_wave_mates(gpu_lib, name, solver):
    """Chain 1 (the wave-mate of chain 0, and of 2 and 3 for one star) starts
    with a NaN flux: exactly the NONFINITE bit, and nobody else moves by more
    than the last bits."""
    capi = gpu_lib
    case = free_case(name, solver)
    q0, p0, n_steps = case["q0"], case["p0"], case["n_steps"]
    qb = q0.copy()
    qb[1, 0] = np.nan
    with _Ctx(capi, name, case) as ctx:
        P = capi.make_params(**case["par"])
        q, p, st = ctx.integrate(P, _sid(capi, solver), q0, p0, n_steps, f_pos=True,
                                 return_status=True)
        q2, p2, st2 = ctx.integrate(P, _sid(capi, solver), qb, p0, n_steps, f_pos=True,
                                    return_status=True)
    assert st2[1] == capi.STATUS_NONFINITE
    assert np.isnan(q2[1, 0])
    others = [c for c in range(len(q0)) if c != 1]
    assert np.array_equal(st2[others], st[others])
    for c in others:
        assert _rel_each(q2[c], q[c]) <= 1e-12 and _rel_each(p2[c], p[c]) <= 1e-12
