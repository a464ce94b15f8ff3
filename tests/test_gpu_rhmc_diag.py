"""RHMC_random_diag on the GPU (samplers.py:668-825; rhmc_diag_random).

* samplers.lightsource_gym.RHMC_random_diag reproduces the chains recorded
  from the reference (tests/golden/rhmc_diag.npz) on every scene.
* The trajectories of every kernel body, chain by chain against the NumPy
  restatement tests/rhmc_diag_ref.py, with and without the flux wall, their
  status words, batch invariance, the trace, a NaN chain beside wave-mates.
* RHMC_random_diag_batched against RHMC_random_diag and the restatement.

Bars.  Trajectories: 1e-10 relative to max|value| + 1 for q and p, the bar of
the HMC_random tests.  The shapes' own conditioning is asserted on the CPU
side first: replaying each chain with the gradient scaled by 1 +- 1e-13 moves
its end state by at most a tenth of that bar, so the bar tests the kernels'
arithmetic.  Chains: A_chain exact, q_chain 1e-10 relative to |value| + 1,
finite E_chain at rtol 1e-11.
"""
import numpy as np
import pytest

from conftest import load_golden
import rhmc_diag_ref
from rhmc_diag_ref import SCENES, ref_of
from rhmc_amd.photometry import mag2flux
from rhmc_amd.samplers import lightsource_gym

pytestmark = pytest.mark.gpu

BAR = 1e-10


def load_scene(name):
    return rhmc_diag_ref.load_scene(load_golden("rhmc_diag"), name)


def _rel(got, want):
    """max |got - want| / (max|want| + 1) (inf when the non-finite entries differ)."""
    got, want = np.asarray(got, dtype=float), np.asarray(want, dtype=float)
    fin = np.isfinite(want)
    if got.shape != want.shape or not np.array_equal(np.isfinite(got), fin):
        return np.inf
    if not fin.any():
        return 0.
    return float(np.abs(got[fin] - want[fin]).max() / (np.abs(want[fin]).max() + 1.))


def _rel_each(got, want):
    """max |got - want| / (|want| + 1) over the finite entries."""
    got, want = np.asarray(got, dtype=float), np.asarray(want, dtype=float)
    fin = np.isfinite(want)
    if got.shape != want.shape or not np.array_equal(np.isfinite(got), fin):
        return np.inf
    return float((np.abs(got[fin] - want[fin]) / (np.abs(want[fin]) + 1.)).max()) if fin.any() \
        else 0.


def _gym(D, f_lim=0.):
    g = lightsource_gym()
    g.num_rows, g.num_cols = D.shape
    g.D = D
    g.f_lim = f_lim
    g.compute_factors()
    return g


# ------------------------------------------------------------------ the chains
@pytest.mark.parametrize("name", SCENES)
def test_chain_reproduces_the_reference(gpu_lib, name, capsys):
    s = load_scene(name)
    g = _gym(s["D"].astype(float))
    assert g.factor1 == float(s["factor1"])
    save = "qs" in s
    np.random.seed(int(s["run_seed"]))
    g.RHMC_random_diag(s["q_model_0"].copy(), Niter=int(s["n_iter"]),
                       steps_min=int(s["steps_min"]), steps_max=int(s["steps_max"]),
                       f_lim=float(s["f_lim"]), dt_global=float(s["dt_global"]), save_traj=save)
    assert np.random.random() == float(s["next_random"])      # the reference's draw order
    assert g.Nobjs == s["q_model_0"].shape[0] and g.d == s["q_model_0"].size
    assert g.q_chain.shape == (1, 41, g.d) and g.A_chain.shape == (1, 40, 1)
    assert np.array_equal(g.A_chain[0, :, 0], s["A_chain"])
    eq = _rel_each(g.q_chain[0], s["q_chain"])
    E, Ew = g.E_chain[0, :, 0], s["E_chain"]
    fin = np.isfinite(Ew)
    assert np.array_equal(np.isinf(E), np.isinf(Ew)) and np.array_equal(np.isfinite(E), fin)
    eE = float((np.abs(E[fin] - Ew[fin]) / np.abs(Ew[fin])).max())
    with capsys.disabled():
        print("\n  %s: q_chain %.3g (bar 1e-10), E_chain %.3g (rtol 1e-11)" % (name, eq, eE))
    assert eq <= BAR
    assert eE <= 1e-11
    if save:
        assert len(g.qs) == len(g.Vs) == len(g.Ts) == 41
        for i, n in enumerate(s["traj_len"]):
            assert g.qs[i].shape == (n, 3) and g.Vs[i].shape == (n,) and g.Ts[i].shape == (n,)
            assert _rel_each(g.qs[i], s["qs"][i, :n]) <= BAR
            assert np.allclose(g.Vs[i], s["Vs"][i, :n], rtol=1e-11, atol=0.)
            assert np.allclose(g.Ts[i], s["Ts"][i, :n], rtol=1e-11, atol=0.)


# ----------------------------------------------------------- the trajectories
# id: K, image side, chains, forced kernel, step, trajectory lengths
CASES = {
    "k1_regwin": (1, 32, 5, None, 0.2, (17, 1, 30, 12, 23)),
    "k1_windowed": (1, 48, 5, "windowed", 0.2, (17, 1, 30, 12, 23)),
    "k3_pixmajor": (3, 48, 5, None, 0.1, (17, 1, 30, 12, 23)),
    "k3_multiwin": (3, 48, 5, "multiwin", 0.1, (17, 1, 30, 12, 23)),
    "k3_multiwin_notab": (3, 48, 5, "multiwin_notab", 0.1, (17, 1, 30, 12, 23)),
    "k12_dense": (12, 32, 3, None, 0.05, (14, 1, 9)),
    "k12_windowed": (12, 32, 3, "windowed", 0.05, (14, 1, 9)),
    "k70_two_slots": (70, 32, 2, None, 0.02, (9, 6)),
    "k40_multiwin_two_slots": (40, 64, 3, None, 0.02, (9, 1, 6)),
}
WALL_MAG = 21.7             # scene `wall`'s flux wall
WALL_STEPS = 40             # the longest wall trajectory looked at
_cache = {}


def _field(K, side, n, seed):
    """A Poisson image of K stars and n chains started near the truth, each
    with a momentum drawn under its own mass matrix."""
    g = lightsource_gym()
    rng = np.random.RandomState(seed)
    mags = rng.uniform(19.5, 21.3, K)
    q_true = np.stack([mag2flux(mags) * g.flux_to_count, rng.uniform(5, side - 5, K),
                       rng.uniform(5, side - 5, K)], axis=1)
    lam = np.ones((side, side)) * g.B_count
    for f, x, y in q_true:
        lam += f * rhmc_diag_ref.gauss_PSF(side, side, x, y, FWHM=g.PSF_FWHM_pix)
    D = rng.poisson(lam).astype(float)
    q0 = np.tile(q_true.reshape(-1), (n, 1))
    q0[:, 0::3] *= np.exp(0.03 * rng.randn(n, K))
    q0[:, 1::3] += 0.2 * rng.randn(n, K)
    q0[:, 2::3] += 0.2 * rng.randn(n, K)
    return D, q0, rng.randn(n, 3 * K)


def _conditioned(r_args, q, p, steps, dt, f_lim, want):
    """The chain's end state under a gradient scaled by 1 +- 1e-13 stays within
    a tenth of the bar (and flips where the unscaled one does)."""
    for sG in (1 + 1e-13, 1 - 1e-13):
        got = rhmc_diag_ref.DiagRef(*r_args, scale_G=sG).traj(q, p, steps, dt, f_lim)
        assert got[2] == want[2]
        assert max(_rel(got[0], want[0]), _rel(got[1], want[1])) <= 0.1 * BAR


def _case(name, wall):
    """(gym, q0, p0, steps, dt, restatement results per chain), computed once."""
    if (name, wall) in _cache:
        return _cache[(name, wall)]
    K, side, n, kernel, dt, steps = CASES[name]
    D, q0, z = _field(K, side, n, 100 + K + side)
    f_lim = 0.
    if wall:        # the faintest star of every chain starts just above the wall, moving down
        f_lim = mag2flux(WALL_MAG) * lightsource_gym().flux_to_count
        faint = 3 * int(np.argmin(q0[0, 0::3]))
        q0[:, faint] = f_lim * (1.02 + 0.01 * np.arange(n))
        z[:, faint] = -2.0 - 0.1 * np.arange(n)
    g = _gym(D, f_lim)
    r_args = (D, g.B_count, g.PSF_FWHM_pix, g.factor1)
    r = rhmc_diag_ref.DiagRef(*r_args)
    p0 = z * np.sqrt(np.array([r.mass_matrix(q) for q in q0]))
    steps = np.array(steps, np.int32)
    if wall:
        # trajectories do not depend on their length: look at WALL_STEPS steps,
        # end even chains ON their first flipped step and odd ones past it
        for c in range(n):
            tr = r.traj(q0[c], p0[c], WALL_STEPS, dt, f_lim)[3]
            below = (tr[1:, 0::3] < f_lim).any(axis=1)
            assert below.any(), (name, c)
            first = int(np.argmax(below)) + 1
            steps[c] = first if c % 2 == 0 else min(first + 4, WALL_STEPS)
            f = tr[:steps[c] + 1, 0::3]
            assert (np.abs(f - f_lim) > 1e-7 * f_lim).all()     # no decision on the edge
    want = [r.traj(q0[c], p0[c], int(steps[c]), dt, f_lim) for c in range(n)]
    for c in range(n):
        _conditioned(r_args, q0[c], p0[c], int(steps[c]), dt, f_lim, want[c])
    _cache[(name, wall)] = (g, q0, p0, steps, dt, want)
    return _cache[(name, wall)]


def _ctx(g, kernel):
    ctx = g._context()
    ctx.set_kernel(kernel or "auto")
    return ctx


@pytest.mark.parametrize("wall", [False, True], ids=["free", "wall"])
@pytest.mark.parametrize("name", list(CASES))
def test_trajectories_status_batch_and_trace(gpu_lib, name, wall, capsys):
    capi = gpu_lib
    g, q0, p0, steps, dt, want = _case(name, wall)
    kernel = CASES[name][3]
    n = len(q0)
    ctx = _ctx(g, kernel)
    P = g._params()
    q, p, st = ctx.diag_random(P, dt, g.factor1, q0, p0, steps, return_status=True)
    worst = 0.
    for c in range(n):
        worst = max(worst, _rel(q[c], want[c][0]), _rel(p[c], want[c][1]))
    with capsys.disabled():
        print("\n  %s %s: worst %.3g of max|value| + 1 (bar 1e-10)" % (
            name, "wall" if wall else "free", worst))
    assert worst <= BAR
    flipped = np.array([w[2] for w in want])
    assert np.array_equal(st, np.where(flipped, capi.STATUS_REFLECT_F, 0))
    assert np.array_equal(p[flipped], p0[flipped])              # the stale momentum
    if wall:
        mid = sum(bool((w[3][1:-1, 0::3] < g.f_lim).any()) for w in want)
        assert flipped.sum() > 0 and mid > 0
    else:           # unequal lengths inside a wave; a one-step chain wherever there are three
        assert len(set(steps)) == n and (n < 3 or steps.min() == 1)
    # batch invariance: a subset gives the same bits
    sub = [0, n - 1] if n > 2 else [n - 1]
    qs, ps, sts = ctx.diag_random(P, dt, g.factor1, q0[sub], p0[sub], steps[sub],
                                  return_status=True)
    assert np.array_equal(qs, q[sub]) and np.array_equal(ps, p[sub], equal_nan=True)
    assert np.array_equal(sts, st[sub])
    # the trace: rows 0 .. steps[c], the rest untouched; the results unchanged
    qt, pt, tr = ctx.diag_random(P, dt, g.factor1, q0, p0, steps, trace=True)
    assert np.array_equal(qt, q) and np.array_equal(pt, p)
    assert tr.shape == (n, steps.max() + 1, q0.shape[1])
    for c in range(n):
        assert np.array_equal(tr[c, 0], q0[c])
        assert _rel(tr[c, :steps[c] + 1], want[c][3]) <= BAR
        assert np.array_equal(tr[c, steps[c]], q[c])
        assert np.isnan(tr[c, steps[c] + 1:]).all()
    ctx.set_kernel("auto")


def test_trace_rows_are_checked(gpu_lib):
    capi = gpu_lib
    g, q0, p0, steps, dt, _ = _case("k1_regwin", False)
    ctx = _ctx(g, None)
    o = capi.DiagOpts(dt, g.factor1, int(steps.max()), 0)      # one row short
    import ctypes
    q, p = q0.copy(), p0.copy()
    tr = np.zeros((len(q0), int(steps.max()), 3))
    vp = ctypes.c_void_p
    rc = capi.lib().rhmc_diag_random(ctx.handle, ctypes.byref(g._params()), ctypes.byref(o),
                                     vp(q.ctypes.data), vp(p.ctypes.data),
                                     vp(steps.ctypes.data), len(q0), 1, None,
                                     vp(tr.ctypes.data))
    assert rc == capi.RHMC_ERR_ARG
    assert b"trace_rows" in capi.lib().rhmc_last_error()
    assert np.array_equal(q, q0) and not tr.any()
    assert ctx.diag_random(g._params(), dt, g.factor1, q0[:0], p0[:0], steps[:0])[0].shape \
        == (0, 3)                                                # no chains: a no-op


@pytest.mark.parametrize("name", ["k1_regwin", "k3_pixmajor", "k3_multiwin", "k12_dense"])
def test_nan_chain_beside_wave_mates(gpu_lib, name):
    """Chain 1 (the wave-mate of chain 0, and of 2 and 3 for one star) starts
    with a NaN flux: exactly the NONFINITE bit, and nobody else moves by more
    than the last bits."""
    capi = gpu_lib
    g, q0, p0, steps, dt, want = _case(name, False)
    ctx = _ctx(g, CASES[name][3])
    P = g._params()
    q, p, st = ctx.diag_random(P, dt, g.factor1, q0, p0, steps, return_status=True)
    qb = q0.copy()
    qb[1, 0] = np.nan
    q2, p2, st2 = ctx.diag_random(P, dt, g.factor1, qb, p0, steps, return_status=True)
    ctx.set_kernel("auto")
    assert st2[1] == capi.STATUS_NONFINITE
    assert np.isnan(q2[1, 0])
    others = [c for c in range(len(q0)) if c != 1]
    assert np.array_equal(st2[others], st[others])
    for c in others:
        assert _rel_each(q2[c], q[c]) <= 1e-12 and _rel_each(p2[c], p[c]) <= 1e-12


# ------------------------------------------------------------------ batched
def test_batched_one_chain_is_the_reference_call(gpu_lib):
    s = load_scene("k3")
    kw = dict(Niter=12, f_lim=float(s["f_lim"]), dt_global=float(s["dt_global"]))
    a, b = _gym(s["D"].astype(float)), _gym(s["D"].astype(float))
    np.random.seed(int(s["run_seed"]))
    a.RHMC_random_diag(s["q_model_0"].copy(), **kw)
    nxt = np.random.random()
    np.random.seed(int(s["run_seed"]))
    b.RHMC_random_diag_batched(s["q_model_0"].reshape(1, -1), **kw)
    assert np.random.random() == nxt
    assert (b.Nchain, b.Nobjs, b.d) == (1, 3, 9)
    for k in ("q_chain", "E_chain", "dE_chain", "A_chain"):
        assert np.array_equal(getattr(a, k), getattr(b, k), equal_nan=True), k
    assert np.array_equal(a.A_chain[0, :, 0], s["A_chain"][:12])


def test_batched_three_chains_against_the_restatement(gpu_lib):
    s = load_scene("k3")
    r = ref_of(s)
    n, d, Niter = 3, 9, 10
    dt, f_lim = float(s["dt_global"]), float(s["f_lim"])
    rng = np.random.RandomState(2)
    q0 = s["q_model_0"].reshape(1, -1) * (1 + 0.01 * rng.randn(n, d))
    np.random.seed(9)                       # the batched draw order
    z = [np.random.randn(n, d)]
    steps, lnu = [], []
    for _ in range(Niter):
        z.append(np.random.randn(n, d))
        steps.append(np.random.randint(low=10, high=50, size=n))
        lnu.append(np.log(np.random.random(n)))
    z, steps, lnu = np.array(z), np.array(steps), np.array(lnu)
    g = _gym(s["D"].astype(float))
    np.random.seed(9)
    g.RHMC_random_diag_batched(q0, Niter=Niter, f_lim=f_lim, dt_global=dt)
    assert g.q_chain.shape == (n, Niter + 1, d) and g.Nchain == n
    for c in range(n):
        run = r.run(q0[c], Niter, dt, f_lim, z=z[:, c], steps=steps[:, c], lnu=lnu[:, c])
        with np.errstate(invalid="ignore"):
            tested = np.isfinite(run["dE"]) & (run["dE"] >= 0)
            assert (np.abs(run["lnu"] + run["dE"])[tested] >= 1e-6).all()   # no edge decisions
        assert np.array_equal(g.A_chain[c, :, 0], run["A_chain"])
        assert _rel_each(g.q_chain[c], run["q_chain"]) <= BAR
        assert np.allclose(g.E_chain[c, :, 0], run["E_chain"], rtol=1e-11, atol=0.)
