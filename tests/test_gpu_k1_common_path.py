"""The one-star step's rare paths (rhmc_k1step.hpp, rhmc_tiledr.hpp).

The step loop keeps its common case as straight-line code: the window reload,
the direct-factor fallback, the three reflection blocks and the second and
later passes of both fixed-point loops sit out of line behind unlikely
branches, the first pass of each loop is peeled, and the closing flux metric
applies `f < f_low` as a select.  Every case below takes one of those paths
and is compared with the CPU oracle at the project's bar (q 1e-9, p 1e-8
relative to |value| + 1, iteration counts and status bits exact):

paths (dt 0.1, delta 1e-6, 40 steps, 8 chains = two waves, prior off and on)
  wave 0  0 an ordinary chain            1 a fast chain (window moves on most steps)
          2 starts just above the flux wall and crosses it
          3 leaves the image through two edges in one step
  wave 1  4 far outside the image (direct factors, reflects on x and y every step)
          5 f < f_low                    6 f crossing f_low inside a q-loop pass
          7 non-finite (f = NaN): status exactly NONFINITE
loops (dt 1.0, on the 32-px image 2.0: its chains need at most 8 q-iterations
  at 1.0; delta 1e-10, 3 steps, 6 chains): second passes of the p-loop
  (2 iterates per pass) and the q-loop (8 per pass); counter_max 1, 2, 3, 8, 9
  puts the cap inside the peeled pass, on its last iterate and in the
  continuation.
ragged: 1, 5 and 6 chains of `paths`.

On 32- and 48-px images, fp32-exact and not (the fp64 pixel cache), through
`leapfrog` on the register-window and the forced lane-group kernels and
through the fused `mh` kernel.  Iteration counts are defined only where no
fixed-point test value lies within a few ulp of delta
(tests/test_gpu_delta_edge.py): the CPU test checks that the oracle keeps
every test value of every case outside delta (1 +- 1e-9), so no case is
excluded, and that each path above is really taken.
"""
import functools

import numpy as np
import pytest

from helpers import assert_state_close
from oracle import rhmc_ref as R
from rhmc_amd import workloads

F, XY, NONFINITE, PCAP, QCAP, NEAR = 8, 16, 1, 2, 4, 32
PATHS = dict(dt=0.1, delta=1e-6, steps=40, chains=8)
LOOPS = dict(dt={32: 2.0, 48: 1.0}, delta=1e-10, steps=3, chains=6)
CAPS = [1, 2, 3, 8, 9, 1000]
IMAGES = [(32, True), (32, False), (48, True), (48, False)]
# kernels by image exactness: the register-window kernel (28- and 32-px
# windows), the lane-group kernel forced at 4 and 1 lanes per chain
KERNELS = {True: ["auto", "regwin32", "lane4", "lane1"], False: ["auto", "lane1_f64"]}
CASES = [(n, e, k) for n, e in IMAGES for k in KERNELS[e]]


@functools.lru_cache(maxsize=None)
def _scene(img, exact, scen, prior=False):
    """(D, params, q0, p0) of a scenario on the img-px workload image."""
    wl = workloads.make("C1" if img == 32 else "C2", n_chains=8)
    D = wl.D if exact else wl.D + 0.1          # 0.1 is not an fp32 value
    edge = img - 1.0
    q0, p0 = wl.q0.copy(), wl.p0.copy()
    if scen == "loops":
        par = dict(wl.params, dt=LOOPS["dt"][img], delta=LOOPS["delta"])
        return D, par, q0[:LOOPS["chains"]], p0[:LOOPS["chains"]]
    par = dict(wl.params, dt=PATHS["dt"], delta=PATHS["delta"], use_prior=bool(prior))
    f_lim, f_low = par["f_lim"], par["f_low"]
    p0[1, 1], p0[1, 2] = 700.0, -600.0                    # fast
    q0[2, 0], p0[2, 0] = f_lim + 1.0, -0.5                # into the flux wall
    q0[3, 1], q0[3, 2] = 0.01, edge - 0.01                # out through two edges
    p0[3, 1], p0[3, 2] = -80.0, 80.0
    q0[4, 1], q0[4, 2] = 300.0, -250.0                    # far
    q0[5, 0], p0[5, 0] = 2.0, 0.01                        # below f_low
    q0[6, 0], p0[6, 0] = f_low + 0.05, -0.2               # crossing f_low
    q0[7, 0] = np.nan                                     # non-finite
    return D, par, q0, p0


@functools.lru_cache(maxsize=None)
def _oracle(img, exact, scen, prior=False, cm=1000):
    """Per chain: final q, p, iteration totals, status word, and what the CPU
    test looks at (window moves, reflections per step, iterations per step,
    steps below f_low, the least |test value / delta - 1|)."""
    D, par, q0, p0 = _scene(img, exact, scen, prior)
    m = R.RefModel(D, dict(par, rows=img, cols=img))
    sc = PATHS if scen == "paths" else LOOPS
    edge, f_lim, delta = img - 1.0, par["f_lim"], sc["delta"]
    out = []
    with np.errstate(all="ignore"):
        for c in range(len(q0)):
            q, p = q0[c].copy(), p0[c].copy()
            st = n_p = n_q = moves = 0
            refl, its, low, margin = [], [], 0, np.inf
            for _ in range(sc["steps"]):
                o = (np.floor(q[1] + .5), np.floor(q[2] + .5))
                tr = {}
                q, p, a, b = m.step(q, p, delta, cm, trace=tr)
                moves += o != (np.floor(q[1] + .5), np.floor(q[2] + .5))
                n_p, n_q = n_p + a, n_q + b
                its.append((a, b))
                if a == cm and tr["dp"][-1] > delta:
                    st |= PCAP
                if b == cm and tr["dq"][-1] > delta:
                    st |= QCAP
                r = (int(q[0] < f_lim), int(q[1] < 0 or q[1] > edge),
                     int(q[2] < 0 or q[2] > edge))
                refl.append(r)
                st |= F * r[0] | XY * (r[1] | r[2])
                low += bool(q[0] < par["f_low"])
                v = np.array(tr["dp"] + tr["dq"])
                v = v[np.isfinite(v)]
                if v.size:
                    margin = min(margin, np.abs(v / delta - 1.0).min())
            if not (np.isfinite(q).all() and np.isfinite(p).all()):
                st |= NONFINITE
            out.append(dict(q=q, p=p, it=(n_p, n_q), st=st, moves=moves, refl=refl, its=its,
                            low=low, margin=margin))
    return out


def _all_oracles():
    for img, exact in IMAGES:
        for prior in (False, True):
            yield ("paths", img, exact, prior, 1000), _oracle(img, exact, "paths", prior)
        for cm in CAPS:
            yield ("loops", img, exact, False, cm), _oracle(img, exact, "loops", False, cm)


def test_oracle_takes_every_path_and_keeps_clear_of_delta():
    """CPU only: no case is excluded by the delta edge, and the scenarios reach
    what they are there for."""
    for key, ref in _all_oracles():
        for c, r in enumerate(ref):
            assert r["margin"] > 1e-9, (key, c, r["margin"])
        if key[0] == "paths":
            steps = PATHS["steps"]
            assert ref[0]["st"] == 0 and ref[0]["moves"] <= steps // 8, key
            assert ref[1]["moves"] > steps // 2, (key, ref[1]["moves"])
            assert ref[2]["st"] & F, key
            assert any(r[1] and r[2] for r in ref[3]["refl"]), key
            assert all(r[1] and r[2] for r in ref[4]["refl"]), key
            assert ref[5]["low"] >= steps // 2 and ref[5]["st"] & F, key
            assert 0 < ref[6]["low"] < steps, key
            assert ref[7]["st"] == NONFINITE and ref[7]["it"] == (steps, steps), key
        else:
            cm = key[4]
            its = np.array([r["its"] for r in ref])          # [chain, step, loop]
            if cm == 1000:   # second passes of both loops
                assert its[:, :, 0].max() > 2 and its[:, :, 1].max() > 8, key
            else:            # the cap cuts the q-loop, and up to 3 the p-loop, somewhere
                assert any(r["st"] & QCAP for r in ref), key
                assert cm > 3 or any(r["st"] & PCAP for r in ref), key


def _leapfrog(capi, kernel, D, par, q0, p0, steps, cm):
    ctx = capi.Context(D, kernel=kernel)
    try:
        P = capi.make_params(**dict(par, counter_max=cm))
        return ctx.leapfrog(P, q0, p0, steps, return_info=True)
    finally:
        ctx.close()


def _compare(tag, got, ref):
    q, p, it, st = got
    for c, r in enumerate(ref[:len(q)]):
        what = "%s chain %d" % (tag, c)
        assert (int(it[c, 0]), int(it[c, 1])) == r["it"], (what, it[c], r["it"])
        assert int(st[c]) == r["st"], (what, int(st[c]), r["st"])
        if r["st"] & NONFINITE:
            continue
        assert_state_close(q[c], r["q"], 1e-9, "q " + what)
        assert_state_close(p[c], r["p"], 1e-8, "p " + what)


@pytest.mark.gpu
@pytest.mark.parametrize("prior", [False, True])
@pytest.mark.parametrize("img,exact,kernel", CASES)
def test_rare_paths(gpu_lib, img, exact, kernel, prior):
    D, par, q0, p0 = _scene(img, exact, "paths", prior)
    ref = _oracle(img, exact, "paths", prior)
    got = _leapfrog(gpu_lib, kernel, D, par, q0, p0, PATHS["steps"], 1000)
    _compare("%d %s %s" % (img, exact, kernel), got, ref)


@pytest.mark.gpu
@pytest.mark.parametrize("n", [1, 5, 6])
@pytest.mark.parametrize("img,exact,kernel", CASES)
def test_ragged_counts(gpu_lib, img, exact, kernel, n):
    D, par, q0, p0 = _scene(img, exact, "paths")
    ref = _oracle(img, exact, "paths")
    got = _leapfrog(gpu_lib, kernel, D, par, q0[:n], p0[:n], PATHS["steps"], 1000)
    assert len(got[0]) == n
    _compare("%d %s %s n=%d" % (img, exact, kernel, n), got, ref)


@pytest.mark.gpu
@pytest.mark.parametrize("cm", CAPS)
@pytest.mark.parametrize("img,exact,kernel", CASES)
def test_peeled_passes_and_caps(gpu_lib, img, exact, kernel, cm):
    D, par, q0, p0 = _scene(img, exact, "loops")
    ref = _oracle(img, exact, "loops", False, cm)
    got = _leapfrog(gpu_lib, kernel, D, par, q0, p0, LOOPS["steps"], cm)
    _compare("%d %s %s cm=%d" % (img, exact, kernel, cm), got, ref)


def _oracle_mh(D, par, img, q0, z, u, steps, delta, cm):
    """One move-0 iteration of run_RHMC (sampler_RHMC.py:1018-1083) per chain
    with the given randoms: (q after the accept test, accepted)."""
    m = R.RefModel(D, dict(par, rows=img, cols=img, fmin=1.0, fmax=1e5))  # V's prior constant
    out = []
    with np.errstate(all="ignore"):
        for c in range(len(q0)):
            H = m.H(q0[c])
            p = z[c] * np.sqrt(H)
            E0 = m.V(q0[c], True) + m.T(p, H)
            q1, p1, _, _ = m.trajectory(q0[c], p, steps, delta, cm, record=False)
            dE = m.V(q1, True) + m.T(p1, m.H(q1)) - E0
            acc = bool(dE < 0 or np.log(u[c]) < -dE)
            out.append((q1 if acc else q0[c], acc))
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("scen,cm", [("paths", 1000), ("loops", 1000), ("loops", 3), ("loops", 9)])
@pytest.mark.parametrize("img,exact", IMAGES)
def test_fused_mh_takes_the_same_paths(gpu_lib, img, exact, scen, cm):
    """The fused MH kernel runs the same step loop: one iteration whose momentum
    draw reproduces the scenario's p0 (z = p0 / sqrt(H)), with a uniform small
    enough that every finite energy difference accepts."""
    capi = gpu_lib
    D, par, q0, p0 = _scene(img, exact, scen)
    sc = PATHS if scen == "paths" else LOOPS
    m = R.RefModel(D, dict(par, rows=img, cols=img))
    with np.errstate(all="ignore"):
        z = np.array([p0[c] / np.sqrt(m.H(q0[c])) for c in range(len(q0))])
    u = np.full(len(q0), 1e-300)
    ctx = capi.Context(D)
    try:
        P = capi.make_params(**dict(par, counter_max=cm))
        got = ctx.mh(P, q0, 1, sc["steps"], f_pos=True, z=z[None], u=u[None])
    finally:
        ctx.close()
    ref = _oracle_mh(D, par, img, q0, z, u, sc["steps"], sc["delta"], cm)
    for c, (qo, acc) in enumerate(ref):
        what = "%d %s %s chain %d" % (img, exact, scen, c)
        assert bool(got["accept"][0, c]) == acc, what
        if np.isfinite(qo).all():
            assert_state_close(got["q"][c], qo, 1e-9, "q " + what)
        else:
            assert np.array_equal(np.isnan(got["q"][c]), np.isnan(qo)), what
