"""RHMC_random on the GPU (rhmc_hess_derivs, rhmc_hess_random,
samplers.lightsource_gym.RHMC_random / RHMC_random_batched) against the NumPy
restatement tests/rhmc_hess_ref.py and the fixture recorded from the reference
(tests/golden/rhmc_hess.npz).

Bars.  Derivative sets: 1e-10 times the restatement's scale of each entry (the
sum over pixels and terms of |term|), the project's gradient bar; V 1e-10
relative.  Trajectories: 1e-10 (|value| + 1) for q and p with the non-finite
entries in the same places, status words and steps_done exact.  Every start
set is conditioned on the CPU first: replaying each chain with the derivative
arrays scaled by 1 +- 1e-13 changes no steps_done and no status word and moves
no end state by more than a tenth of the bar, so the bar tests the arithmetic.
Chains: A_chain exact, q_chain 1e-10 relative to |value| + 1, finite E_chain at
rtol 1e-11, the bars tests/test_gpu_rhmc_diag.py puts on the same quantities."""
import functools

import numpy as np
import pytest

from conftest import load_golden
import rhmc_hess_ref
from rhmc_hess_ref import STATUS_NONFINITE, STATUS_REFLECT_F, STATUS_REFLECT_XY
from rhmc_amd.photometry import default_exp_setup, gauss_PSF, mag2flux
from rhmc_amd.samplers import lightsource_gym

pytestmark = pytest.mark.gpu

SCENES = rhmc_hess_ref.SCENES
SHAPES = [(1, 16), (1, 32), (2, 32), (3, 48), (10, 48), (16, 48)]     # (K, side)
BAR = 1e-10
SENS_BAR = 0.1 * BAR
DT_F, DT_XY = 0.1, 0.3
N_CHAINS = 9            # the batch; 1, 4 and 5 are its leading rows


def load_scene(name):
    return rhmc_hess_ref.load_scene(load_golden("rhmc_hess"), name)


def _rel_each(got, want):
    """max |got - want| / (|want| + 1) over the finite entries; inf when the
    non-finite entries are not the same ones."""
    got, want = np.asarray(got, dtype=float), np.asarray(want, dtype=float)
    fin = np.isfinite(want)
    if got.shape != want.shape or not np.array_equal(got[~fin], want[~fin], equal_nan=True) \
            or not np.isfinite(got[fin]).all():
        return np.inf
    return float((np.abs(got[fin] - want[fin]) / (np.abs(want[fin]) + 1.)).max()) if fin.any() \
        else 0.


def _params(gpu_lib, B_count, fwhm_pix, f_lim):
    return gpu_lib.make_params(dt=1., delta=1e-6, counter_max=1000, B_count=B_count,
                               f_lim=f_lim, f_low=1., fwhm_pix=fwhm_pix, g_xx=1., g_ff=1.,
                               g_ff2=1., g0=1., g1=1., g2=1.)


# ------------------------------------------------------------------ the images
@functools.lru_cache(maxsize=None)
def image(K, side, edge=False):
    """A Poisson image of K stars on a side x side field (at least 3.5 px from
    the edge), the restatement on it, q_true.  Stars 0 and K - 1 have magnitude
    20.5 and are the faintest, the others 19..20.3: the `wall` set puts the wall
    just below those two.  edge: star 0 lies 0.35 px inside the far edge in x,
    for the `edge` set."""
    rows, cols, flux_to_count, fwhm, B_count = default_exp_setup()[:5]
    rng = np.random.RandomState(1000 * side + K)
    q_true = np.zeros((K, 3))
    mag = rng.uniform(19., 20.3, K)
    mag[0] = mag[K - 1] = 20.5
    q_true[:, 0] = mag2flux(mag) * flux_to_count
    q_true[:, 1:] = rng.uniform(3.5, side - 3.5, (K, 2))
    if edge:
        q_true[0, 1] = side - 0.35
    model = np.ones((side, side)) * B_count
    for f, x, y in q_true:
        model += f * gauss_PSF(side, side, x, y, FWHM=fwhm)
    D = rng.poisson(model).astype(float)
    return D, rhmc_hess_ref.HessRef(D, B_count, fwhm), q_true, B_count, fwhm


def max_steps(K):
    return 50 if K <= 3 else 14


def _momentum(ref, rng, q):
    return rng.randn(q.size) * np.sqrt(np.abs(ref.derivs(q)[1]))


def _near_truth(rng, q_true):
    return (q_true * (1. + 0.05 * rng.randn(len(q_true), 1) * np.array([1., 0., 0.]))
            + 0.3 * rng.randn(len(q_true), 3) * np.array([0., 1., 1.])).reshape(-1)


@functools.lru_cache(maxsize=None)
def start_set(kind, K, side):
    """(q [9, 3K], p, steps [9], f_lim) of one start set, not yet conditioned."""
    D, ref, q_true, _, _ = image(K, side, kind == "edge")
    rng = np.random.RandomState(7 * side + K + {"free": 0, "wall": 100, "edge": 200,
                                                  "neg": 300}[kind])
    n, nmax = N_CHAINS, max_steps(K)
    q = np.array([_near_truth(rng, q_true) for _ in range(n)])
    steps = rng.randint(max(nmax // 3, 2), nmax + 1, n).astype(np.int32)
    if kind in ("edge", "neg"):     # what they test happens in the first steps
        steps = rng.randint(2, 5, n).astype(np.int32)
    f_lim = 0.
    if kind == "neg":   # star 0 moved onto empty sky: the model overshoots there
        sky = _empty_sky(D, q_true, side)
        q[:, 1], q[:, 2] = sky[0] + 0.2 * rng.randn(n), sky[1] + 0.2 * rng.randn(n)
    p = np.array([_momentum(ref, rng, row) for row in q])
    if kind in ("edge", "neg"):     # gentle: a star off its data runs away within a few steps
        p *= 0.3
    if kind == "edge":  # star 0 at 0.05..0.6 px from the far edge, 0.3 px per step outwards
        q[:, 1] = side - np.linspace(0.05, 0.6, n)
        for c in range(n):
            p[c, 1] = 0.3 / DT_XY * ref.derivs(q[c])[1][1]
    if kind == "wall":
        # the wall 15% below the two faintest stars; the designated one (K - 1
        # in even chains, 0 in odd ones) starts 12% above the wall and loses
        # about 4% of the wall's flux per step
        f_lim = 0.85 * q_true[0, 0]
        for c in range(n - 1):
            star = (K - 1) if c % 2 == 0 else 0
            q[c, 0::3] = np.maximum(q[c, 0::3], 1.3 * f_lim)
            q[c, 3 * star] = 1.12 * f_lim
            p[c] = _momentum(ref, rng, q[c])
            p[c, 0::3] = np.abs(p[c, 0::3])
            p[c, 3 * star] = -0.04 * f_lim / DT_F * ref.derivs(q[c])[1][3 * star]
            dt = np.asarray([DT_F, DT_XY, DT_XY] * K)
            t = ref.traj(q[c].copy(), p[c].copy(), nmax - 4, dt, f_lim)
            crossed = t["steps_done"]       # the crossing is on step `crossed` (1-based)
            assert t["diverged_at"] is not None and crossed >= 1, (kind, K, side, c)
            steps[c] = crossed if c % 2 == 0 else crossed + 4
        q[n - 1, 0] = 0.5 * f_lim           # the last chain starts below the wall
    return q, p, steps, f_lim


def _empty_sky(D, q_true, side):
    """The pixel centre farthest from every star, at least 4 px inside."""
    best, where = -1., None
    for i in range(4, side - 4):
        for j in range(4, side - 4):
            dist = np.min(np.hypot(q_true[:, 1] - (i + .5), q_true[:, 2] - (j + .5)))
            if dist > best:
                best, where = dist, (i + .5, j + .5)
    return where


@functools.lru_cache(maxsize=None)
def conditioned(kind, K, side):
    """The start set with the restatement's trajectories, after the CPU
    conditioning assertions."""
    D, ref, q_true, B_count, fwhm = image(K, side, kind == "edge")
    q, p, steps, f_lim = start_set(kind, K, side)
    dt = np.asarray([DT_F, DT_XY, DT_XY] * K)

    def run(r):
        return [r.traj(q[c].copy(), p[c].copy(), int(steps[c]), dt, f_lim)
                for c in range(len(q))]
    want = run(ref)
    worst = 0.
    for sG in (1 + 1e-13, 1 - 1e-13):
        got = run(rhmc_hess_ref.HessRef(D, B_count, fwhm, scale_G=sG))
        for c, (a, b) in enumerate(zip(got, want)):
            assert a["steps_done"] == b["steps_done"] and a["status"] == b["status"], (kind, c)
            worst = max(worst, _rel_each(a["q"], b["q"]), _rel_each(a["p"], b["p"]))
    assert worst <= SENS_BAR, (kind, K, side, worst)
    done = np.array([t["steps_done"] for t in want])
    status = np.array([t["status"] for t in want])
    if kind == "free":
        assert (done == steps).all()
    if kind == "wall":
        n = len(q)
        even, odd = np.arange(0, n - 1, 2), np.arange(1, n - 1, 2)
        assert (done[even] == steps[even]).all() and (done[odd] == steps[odd] - 4).all()
        assert done[n - 1] == 0 and (status[:n - 1] & STATUS_REFLECT_F).all()
        # the crossing leaves infinities in p wherever no flag is set: the
        # other stars' flux momenta (none with K = 1), and all of p in the last chain
        for c in range(n):
            assert np.isinf(want[c]["p"]).any() == (K > 1 or c == n - 1)
            assert bool(status[c] & STATUS_NONFINITE) == (K > 1 or c == n - 1)
    if kind == "edge":
        # chains that leave on the first step (x >= side) take the force update
        # there; with K = 2 the other star keeps the switch on
        first = [ref.traj(q[c].copy(), p[c].copy(), 1, dt, f_lim) for c in range(len(q))]
        left = np.array([t["q"][1] >= side for t in first])
        assert left.any() and not left.all()
        for c in np.flatnonzero(left):
            assert first[c]["p"][1] != -(p[c, 1] + dt[1] * ref.compute(
                q[c], p[c], f_lim)[1][1] / 2.)
        assert (status & STATUS_REFLECT_XY).all()
    if kind == "neg":
        assert all((ref.derivs(row)[1] < 0).any() for row in q)
    return q, p, steps, f_lim, want


# ------------------------------------------------------------- derivative sets
def _check_derivs(ref, q, got, V, capsys, label):
    worst = [0., 0., 0.]
    for c in range(len(q)):
        w1, w2, w3, scales = ref.derivs(q[c], scales=True)
        for m, (g, w, sc) in enumerate(zip(got, (w1, w2, w3), scales)):
            worst[m] = max(worst[m], float(np.max(np.abs(g[c] - w) / sc)))
    eV = max(abs(V[c] - ref.V(q[c])) / abs(ref.V(q[c])) for c in range(len(q)))
    with capsys.disabled():
        print("\n  %s: dVdq %.3g dVdqq %.3g dVdqqq %.3g of the scale, V %.3g (bars 1e-10)"
              % ((label,) + tuple(worst) + (eV,)))
    assert max(worst) <= BAR and eV <= 1e-10


@pytest.mark.parametrize("K,side", SHAPES)
def test_derivs_against_the_restatement(gpu_lib, K, side, capsys):
    D, ref, q_true, B_count, fwhm = image(K, side)
    rng = np.random.RandomState(K + side)
    q = np.array([_near_truth(rng, q_true) for _ in range(5)])
    ctx = gpu_lib.Context(D, device=0)
    P = _params(gpu_lib, B_count, fwhm, 0.)
    d1, d2, d3, V = ctx.hess_derivs(P, q, V=True)
    _check_derivs(ref, q, (d1, d2, d3), V, capsys, "K=%d %dpx" % (K, side))
    # without V the same bits; one chain in 1-D form
    e1, e2, e3 = ctx.hess_derivs(P, q)
    assert np.array_equal(e1, d1) and np.array_equal(e2, d2) and np.array_equal(e3, d3)
    s1, s2, s3, sV = ctx.hess_derivs(P, q[3], V=True)
    assert np.array_equal(s2, d2[3]) and np.array_equal(s3, d3[3]) and sV == V[3]
    ctx.close()


@pytest.mark.parametrize("name", rhmc_hess_ref.FUNCTIONS)
def test_derivs_against_the_recorded_functions(gpu_lib, name, capsys):
    """RHMC_efficient_computation as recorded from the reference: dVdqq against
    the record itself, the three sets and V against the restatement, and the
    gym's method in its three return shapes."""
    s = load_scene(name)
    ref = rhmc_hess_ref.ref_of(s)
    D = s["D"].astype(float)
    ctx = gpu_lib.Context(D, device=0)
    P = _params(gpu_lib, float(s["B_count"]), float(s["fwhm_pix"]), float(s["f_lim"]))
    d1, d2, d3, V = ctx.hess_derivs(P, s["q"], V=True)
    _check_derivs(ref, s["q"], (d1, d2, d3), V, capsys, name)
    for c in range(len(s["q"])):
        sc = ref.derivs(s["q"][c], scales=True)[3][1]
        assert (np.abs(d2[c] - s["dVdqq"][c]) <= BAR * sc).all()
    ctx.close()
    g = lightsource_gym()
    g.num_rows = g.num_cols = int(s["side"])
    g.B_count, g.PSF_FWHM_pix = float(s["B_count"]), float(s["fwhm_pix"])
    g.D = D
    g.f_lim = float(s["f_lim"])
    n = len(s["q"])
    assert g.RHMC_efficient_computation(s["q"][n - 1], s["p"][n - 1]) == (np.inf,) * 3
    h = g.RHMC_efficient_computation(s["q"][n - 1], s["p"][n - 1], dVdqq_only=True)
    assert np.array_equal(h, d2[n - 1])
    dqdt, dpdt, E = g.RHMC_efficient_computation(s["q"][0], s["p"][0], debug=False)
    assert np.allclose(dqdt, s["dqdt"][0], rtol=1e-9, atol=0.)
    assert abs(E - s["E"][0]) <= 1e-10 * abs(s["E"][0])


def test_unserved_shapes_are_refused(gpu_lib):
    D, _, q_true, B_count, fwhm = image(1, 16)
    P = _params(gpu_lib, B_count, fwhm, 0.)
    ctx = gpu_lib.Context(D, device=0)
    q17 = np.tile(q_true.reshape(-1), 17)[None]
    with pytest.raises(gpu_lib.RhmcError) as e:
        ctx.hess_derivs(P, q17)
    assert e.value.code == gpu_lib.RHMC_ERR_UNSUPPORTED
    with pytest.raises(gpu_lib.RhmcError) as e:
        ctx.hess_random(P, DT_F, DT_XY, q17, np.zeros_like(q17), 3)
    assert e.value.code == gpu_lib.RHMC_ERR_UNSUPPORTED
    ctx.close()
    for side in (15, 49):
        ctx = gpu_lib.Context(np.full((side, side), 25.), device=0)
        with pytest.raises(gpu_lib.RhmcError) as e:
            ctx.hess_derivs(P, q_true.reshape(1, -1))
        assert e.value.code == gpu_lib.RHMC_ERR_UNSUPPORTED
        ctx.close()


# ---------------------------------------------------------------- trajectories
CASES = [("free", K, side) for K, side in SHAPES] + [("wall", K, side) for K, side in SHAPES] \
    + [("edge", 1, 16), ("edge", 1, 32), ("edge", 2, 32), ("neg", 1, 32), ("neg", 3, 48)]


@pytest.mark.parametrize("kind,K,side", CASES)
def test_trajectories(gpu_lib, kind, K, side, capsys):
    """Chain counts 9, 5, 4 and 1 against hess_ref.traj; the smaller batches
    are the leading rows of the 9, bit for bit; the derivative sets written at
    the end state are rhmc_hess_derivs there, bit for bit."""
    D, ref, _, B_count, fwhm = image(K, side, kind == "edge")
    q, p, steps, f_lim, want = conditioned(kind, K, side)
    assert steps.max() <= 50
    ctx = gpu_lib.Context(D, device=0)
    P = _params(gpu_lib, B_count, fwhm, f_lim)
    full = ctx.hess_random(P, DT_F, DT_XY, q, p, steps, derivs=True)
    q2, p2, st, done = full[:4]
    eq = max(_rel_each(q2[c], want[c]["q"]) for c in range(len(q)))
    ep = max(_rel_each(p2[c], want[c]["p"]) for c in range(len(q)))
    with capsys.disabled():
        print("\n  %s K=%d %dpx: q %.3g p %.3g of |value| + 1 (bar 1e-10)"
              % (kind, K, side, eq, ep))
    assert np.array_equal(done, [t["steps_done"] for t in want])
    assert np.array_equal(st, [t["status"] for t in want])
    assert eq <= BAR and ep <= BAR
    for n in (5, 4, 1):
        part = ctx.hess_random(P, DT_F, DT_XY, q[:n], p[:n], steps[:n], derivs=True)
        for a, b in zip(part, full):
            assert np.array_equal(a, b[:n], equal_nan=True), n
    ends = ctx.hess_derivs(P, q2)
    for a, b in zip(full[4:], ends):
        assert np.array_equal(a, b, equal_nan=True)
    # the inputs are not touched, a 1-D call is the chain alone
    one = ctx.hess_random(P, DT_F, DT_XY, q[2], p[2], steps[2])
    assert np.array_equal(one[0], q2[2], equal_nan=True) and one[3] == done[2]
    ctx.close()


@pytest.mark.parametrize("K,side", [(2, 32), (16, 48)])
def test_nan_chain_beside_workgroup_mates(gpu_lib, K, side):
    """A chain whose state is NaN leaves the chains of its workgroup (four
    waves at K = 2, two at K = 16 on 48 px) bit-identical."""
    D, _, _, B_count, fwhm = image(K, side)
    q, p, steps, f_lim, _ = conditioned("free", K, side)
    ctx = gpu_lib.Context(D, device=0)
    P = _params(gpu_lib, B_count, fwhm, f_lim)
    base = ctx.hess_random(P, DT_F, DT_XY, q, p, steps, derivs=True)
    qn, pn = q.copy(), p.copy()
    qn[1, 1] = np.nan
    pn[6, 0] = np.nan
    got = ctx.hess_random(P, DT_F, DT_XY, qn, pn, steps, derivs=True)
    others = [c for c in range(len(q)) if c not in (1, 6)]
    for a, b in zip(got, base):
        assert np.array_equal(a[others], b[others], equal_nan=True)
    assert got[2][1] & STATUS_NONFINITE and got[2][6] & STATUS_NONFINITE
    assert np.isnan(got[0][1]).any() and np.isnan(got[1][6]).any()
    ctx.close()


# ---------------------------------------------------------------------- chains
def _gym(s):
    g = lightsource_gym()
    g.num_rows = g.num_cols = int(s["side"])
    g.B_count, g.PSF_FWHM_pix = float(s["B_count"]), float(s["fwhm_pix"])
    g.D = s["D"].astype(float)
    return g


def _kwargs(s):
    return dict(Niter=int(s["n_iter"]), steps_min=int(s["steps_min"]),
                steps_max=int(s["steps_max"]), f_lim=float(s["f_lim"]),
                dt_RHMC_xy=float(s["dt_xy"]), dt_RHMC_f=float(s["dt_f"]))


def _chain_errors(g, c, want_q, want_E):
    eq = _rel_each(g.q_chain[c], want_q)
    E = g.E_chain[c, :, 0]
    fin = np.isfinite(want_E) & (want_E != 0)
    assert np.array_equal(E[~fin], want_E[~fin], equal_nan=True)
    eE = float((np.abs(E[fin] - want_E[fin]) / np.abs(want_E[fin])).max())
    return eq, eE


@pytest.mark.parametrize("name", SCENES)
def test_chain_reproduces_the_reference(gpu_lib, name, capsys):
    s = load_scene(name)
    g = _gym(s)
    q0 = s["q_model_0"].copy()
    np.random.seed(int(s["run_seed"]))
    g.RHMC_random(q0, **_kwargs(s))
    assert np.random.random() == float(s["next_random"])      # the reference's draw order
    out = capsys.readouterr().out.splitlines()
    n, niter = int(s["n_run"]), int(s["n_iter"])
    assert g.Nobjs == q0.shape[0] and g.d == q0.size
    assert g.q_chain.shape == (1, niter + 1, g.d) and g.A_chain.shape == (1, niter, 1)
    assert np.array_equal(g.A_chain[0, :, 0], s["A_chain"])
    eq, eE = _chain_errors(g, 0, s["q_chain"], s["E_chain"])
    with capsys.disabled():
        print("\n  %s: q_chain %.3g (bar 1e-10), E_chain %.3g (rtol 1e-11)" % (name, eq, eE))
    assert eq <= BAR
    assert eE <= 1e-11
    assert out == list(s["lines"])
    # the caller's array is overwritten; rows past an early stop stay zero
    assert np.array_equal(q0.reshape(-1), g.q_chain[0, n], equal_nan=True)
    assert not g.q_chain[0, n + 1:].any()


def test_batched_one_chain_is_the_reference_call(gpu_lib):
    s = load_scene("k3")
    g, h = _gym(s), _gym(s)
    np.random.seed(int(s["run_seed"]))
    g.RHMC_random(s["q_model_0"].copy(), **_kwargs(s))
    q0 = s["q_model_0"].reshape(1, -1).copy()
    np.random.seed(int(s["run_seed"]))
    h.RHMC_random_batched(q0, **_kwargs(s))
    assert np.random.random() == float(s["next_random"])
    for k in ("q_chain", "E_chain", "dE_chain", "A_chain"):
        assert np.array_equal(getattr(g, k), getattr(h, k), equal_nan=True), k
    assert np.array_equal(q0[0], h.q_chain[0, -1])


def test_batched_three_chains_against_the_restatement(gpu_lib, capsys):
    s = load_scene("k3")
    kw = _kwargs(s)
    kw["Niter"] = 12
    d = s["q_model_0"].size
    rng = np.random.RandomState(5)
    starts = np.array([_near_truth(rng, s["q_true"]) for _ in range(3)])
    np.random.seed(4321)
    z, steps, lnu = np.zeros((13, 3, d)), np.zeros((12, 3), np.int32), np.zeros((12, 3))
    for i in range(13):
        z[i] = np.random.randn(3, d)
        if i:
            steps[i - 1] = np.random.randint(low=kw["steps_min"], high=kw["steps_max"], size=3)
            lnu[i - 1] = np.log(np.random.random(3))
    nxt = np.random.random()
    g = _gym(s)
    q0 = starts.copy()
    np.random.seed(4321)
    g.RHMC_random_batched(q0, **kw)
    assert np.random.random() == nxt
    for c in range(3):
        qc = starts[c].copy()
        args = (12, kw["dt_RHMC_f"], kw["dt_RHMC_xy"], kw["f_lim"])
        run = rhmc_hess_ref.ref_of(s).run(qc, *args, z=z[:, c], steps=steps[:, c],
                                          lnu=lnu[:, c])
        with np.errstate(invalid="ignore"):
            tested = np.isfinite(run["dE"]) & (run["dE"] >= 0)
            assert (np.abs(run["lnu"] + run["dE"])[tested] >= 1e-6).all()   # no edge decisions
        for sG in (1 + 1e-13, 1 - 1e-13):       # conditioned like the fixture's scenes
            r2 = rhmc_hess_ref.ref_of(s, scale_G=sG).run(starts[c].copy(), *args, z=z[:, c],
                                                         steps=steps[:, c], lnu=lnu[:, c])
            assert np.array_equal(r2["A_chain"], run["A_chain"])
            assert _rel_each(r2["q_chain"], run["q_chain"]) <= SENS_BAR
        assert np.array_equal(g.A_chain[c, :, 0], run["A_chain"]), c
        eq, eE = _chain_errors(g, c, run["q_chain"], run["E_chain"])
        with capsys.disabled():
            print("\n  chain %d: q_chain %.3g (bar 1e-10), E_chain %.3g (rtol 1e-11)"
                  % (c, eq, eE))
        assert eq <= BAR and eE <= 1e-11
        assert np.array_equal(q0[c], g.q_chain[c, -1])      # the caller's array is overwritten
