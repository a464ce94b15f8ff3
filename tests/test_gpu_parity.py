"""GPU parity: the HIP path (through the C-ABI) against the reference goldens
and the CPU oracle.

Tolerances (fp64): gradients and energies to 1e-10 relative to the value
scale; one step to 1e-11; trajectories to 1e-9 (q) / 1e-8 (p) relative to
|value|+1 after up to 500 steps (SURVEY §8(c) measured that 1e-15 input
perturbations grow to <= 8e-12 / 1.3e-10 over 500 steps).  Fixed-point
iteration counts must match the reference exactly on every step.
"""
import numpy as np
import pytest

from conftest import load_golden
from helpers import assert_state_close, capi_params
from oracle import rhmc_ref as R

pytestmark = pytest.mark.gpu


def _ctx(capi, z):
    return capi.Context(z["D"])


KERNEL_PATHS = ["auto", "generic", "windowed", "multiwin", "multiwin_notab", "pixmajor",
                "regwin", "regwin32", "regwin_f64", "lane1", "lane4", "lane1_f64", "dense"]


@pytest.fixture(params=KERNEL_PATHS)
def kernel_path(request, monkeypatch):
    """Run a test on the automatically chosen kernel, then again with every
    context it creates forced onto each kernel family (RHMC_OPT_KERNEL; a
    family that does not serve a case leaves the automatic choice, so many of
    the thirteen runs repeat the automatic body).  Which bodies of the
    implicit step the traj_* goldens reach this way (the keys of
    tests/test_step_bodies.py, from tests/native/traj_bodies.cpp): on the
    one-star goldens (32 and 48 px, fp32-exact, at most 8 chains)
    regwin1/{32,48}/28/float automatically, regwin1/../32/float (regwin32),
    regwin1/../28/double (regwin_f64), lane/../float/{1,4} and
    lane/../double/1 (lane1, lane4, lane1_f64), ldsimage/1, slotted/WinG/1 and
    slotted/Dense{32,48}/1, while pixmajor, multiwin and multiwin_notab leave
    regwin1; on traj_c3, traj_prior and traj_vc (K = 10, 3, 5) pixmajor/{48,32}
    automatically (traj_vc, whose pair potential the pixel-major kernel does
    not serve: multiwin/float/1/tab), multiwin/float/1/tab,
    multiwin/float/1/notab/4, ldsimage/{16,4,8}, slotted/WinG/1 and
    slotted/Dense{48,32}/1, while the six one-star values leave the automatic
    body; on traj_c5 (K = 64, 256 px) multiwin/float/2/notab/4 under eleven
    values and slotted/WinG/1 under generic and windowed.  That is 24 of the 64
    bodies: no fp64 cache but the forced one-star ones, no side of 64, 96 or
    128 px, no window split but 4.  tests/test_gpu_step_bodies.py runs all 64,
    and tests/test_gpu_ragged_bodies.py the 13 a ragged set can launch
    (rhmc_leapfrog_ragged_device; the pixel-major kernel's RAGGED instantiations
    among them, which no fixed-K call reaches).

    Which bodies of rhmc_energy and rhmc_gradient test_gradient_and_energy
    reaches (the keys of tests/test_energy_bodies.py, from the program's
    `energy` and `gradient` modes; all four goldens are fp32-exact, 6 chains):
    the energy of k1 and k1gff2 (48 px) regwin1/48/float under ten values,
    ldsimage/1 (generic), slotted/WinEG/1 (windowed), slotted/Dense48/1
    (dense); of k10 (48 px) ldsimage/16 under eleven values, slotted/WinEG/1
    and slotted/Dense48/1; of vc5 (K = 5, 32 px, the pair potential)
    ldsimage/8, slotted/WinEG/1 and slotted/Dense32/1: 7 of the 22 bodies.
    The gradient takes ldsimage/{1,16,8}, slotted/WinG/1 (windowed) and
    slotted/Dense{48,32}/1 (dense): 6 of the 16.  No fp64 one-star energy, no
    side of 64 px, no ldsimage/2 or /4, nothing with two or more star slots.
    tests/test_gpu_energy_bodies.py runs all 22 and 16, and the 8 + 2 of
    rhmc_mh."""
    from rhmc_amd import capi
    monkeypatch.setattr(capi, "DEFAULT_KERNEL", request.param)
    return request.param




@pytest.mark.parametrize("name", ["k1", "k1gff2", "k10", "vc5"])
def test_gradient_and_energy(gpu_lib, kernel_path, name):
    capi = gpu_lib
    z = load_golden("functions")
    par = R.params_from_npz(z, name + "/par_")
    ctx = capi.Context(z[name + "/D"])
    P = capi_params(capi, par)
    q, p = z[name + "/q"], z[name + "/p"]
    for kind, key in ((0, "dVdq"), (1, "dphidq")):
        g = ctx.gradient(P, q, kind=kind)
        want = z[name + "/" + key]
        scale = np.abs(want).max(axis=1, keepdims=True) + 1.0
        np.testing.assert_array_less(np.abs(g - want) / scale, 1e-10)
    V, T = ctx.energy(P, q, p, f_pos=False)
    np.testing.assert_allclose(V, z[name + "/V"], rtol=1e-12)
    np.testing.assert_allclose(T, z[name + "/T"], rtol=1e-12, atol=1e-12)
    Vp, _ = ctx.energy(P, q, None, f_pos=True)
    want = z[name + "/Vpos"]
    assert np.array_equal(np.isinf(Vp), np.isinf(want))
    fin = np.isfinite(want)
    np.testing.assert_allclose(Vp[fin], want[fin], rtol=1e-12)


def test_single_steps(gpu_lib):
    capi = gpu_lib
    z = load_golden("steps")
    par = R.params_from_npz(z)
    ctx = _ctx(capi, z)
    P = capi_params(capi, par)
    q1, p1, it, st = ctx.leapfrog(P, z["q0"], z["p0"], 1, return_info=True)
    np.testing.assert_array_equal(it[:, 0], z["n_p"])
    np.testing.assert_array_equal(it[:, 1], z["n_q"])
    assert_state_close(q1, z["q1"], 1e-11, "q")
    assert_state_close(p1, z["p1"], 1e-10, "p")
    # the status word reports the reflections that fired
    m = R.RefModel(z["D"], par)
    for c in range(len(q1)):
        refl_f = z["q1"][c, 0] < par["f_lim"]
        assert bool(st[c] & capi.STATUS_REFLECT_F) == refl_f


# (golden, q tol, p tol, free-running horizon).  traj_c3 (K=10, big-sim4
# parameters, stars wandering through the edges) is chaotic: the reference
# itself, started 1e-15 away, leaves 1e-9 agreement after ~130 steps
# (measured with the oracle), so its free-running comparison stops at 100
# steps; every one of its 300 steps is still checked locally (reset to the
# golden state each step).
TRAJ = [("traj_c1", 1e-9, 1e-8, None), ("traj_c2", 1e-9, 1e-8, None),
        ("traj_gff2", 1e-9, 1e-8, None), ("traj_c3", 1e-9, 1e-8, 100),
        ("traj_prior", 1e-9, 1e-8, None), ("traj_vc", 1e-9, 1e-8, None),
        ("traj_edge", 1e-9, 1e-8, None), ("traj_cmax", 1e-9, 1e-8, None),
        ("traj_c5", 1e-9, 1e-8, None)]


@pytest.mark.parametrize("name,qtol,ptol,horizon", TRAJ)
def test_trajectory_stepwise(gpu_lib, name, qtol, ptol, horizon):
    """Every step of the reference trajectory, one launch per step, each
    started from the reference's own state: local error <= 1e-11 and the
    exact fixed-point iteration counts."""
    capi = gpu_lib
    z = load_golden(name)
    par = R.params_from_npz(z)
    ctx = _ctx(capi, z)
    P = capi_params(capi, par, float(z["delta"]), int(z["counter_max"]))
    Q, Pm = z["Q"], z["P"]
    nsteps = Q.shape[1] - 1
    for s in range(nsteps):
        q, p, it, _ = ctx.leapfrog(P, Q[:, s], Pm[:, s], 1, return_info=True)
        np.testing.assert_array_equal(it[:, 0], z["n_p"][:, s], err_msg="p-iters step %d" % s)
        np.testing.assert_array_equal(it[:, 1], z["n_q"][:, s], err_msg="q-iters step %d" % s)
        assert_state_close(q, Q[:, s + 1], 1e-11, "%s q step %d" % (name, s))
        assert_state_close(p, Pm[:, s + 1], 1e-10, "%s p step %d" % (name, s))


@pytest.mark.parametrize("name,qtol,ptol,horizon", TRAJ)
def test_trajectory_fused(gpu_lib, kernel_path, name, qtol, ptol, horizon):
    """Free-running: all steps fused in one launch (the production path)."""
    capi = gpu_lib
    z = load_golden(name)
    par = R.params_from_npz(z)
    ctx = _ctx(capi, z)
    P = capi_params(capi, par, float(z["delta"]), int(z["counter_max"]))
    Q, Pm = z["Q"], z["P"]
    nsteps = Q.shape[1] - 1 if horizon is None else horizon
    q, p, it, st = ctx.leapfrog(P, Q[:, 0], Pm[:, 0], nsteps, return_info=True)
    np.testing.assert_array_equal(it[:, 0], z["n_p"][:, :nsteps].sum(1))
    np.testing.assert_array_equal(it[:, 1], z["n_q"][:, :nsteps].sum(1))
    assert_state_close(q, Q[:, nsteps], qtol, name + " q")
    assert_state_close(p, Pm[:, nsteps], ptol, name + " p")
    assert not (st & capi.STATUS_NONFINITE).any()


def test_chains_independent(gpu_lib, kernel_path):
    """A batch gives exactly the per-chain results (no cross-chain coupling)."""
    capi = gpu_lib
    z = load_golden("traj_c2")
    par = R.params_from_npz(z)
    ctx = _ctx(capi, z)
    P = capi_params(capi, par)
    rs = np.random.RandomState(3)
    n = 37
    q0 = np.repeat(z["Q"][:, 0], 5, axis=0)[:n] * (1 + 1e-3 * rs.randn(n, 3))
    p0 = np.repeat(z["P"][:, 0], 5, axis=0)[:n]
    qb, pb = ctx.leapfrog(P, q0, p0, 20)
    for c in (0, 5, 17, 36):
        qs, ps = ctx.leapfrog(P, q0[c], p0[c], 20)
        assert np.array_equal(qs, qb[c]) and np.array_equal(ps, pb[c])


def test_oracle_matches_gpu_random_chains(gpu_lib, kernel_path):
    """Seeded random chains at C2 geometry: GPU vs the CPU oracle, 100 steps."""
    capi = gpu_lib
    z = load_golden("traj_c2")
    par = R.params_from_npz(z)
    ctx = _ctx(capi, z)
    P = capi_params(capi, par)
    m = R.RefModel(z["D"], par)
    rs = np.random.RandomState(21)
    n = 6
    q0 = np.tile(z["Q"][0, 0], (n, 1)) * np.array([1, 0, 0]) + np.c_[
        z["Q"][0, 0, 0] * np.exp(0.2 * rs.randn(n)), 24 + rs.randn(n), 24 + rs.randn(n)]
    p0 = rs.randn(n, 3) * np.sqrt(np.array([m.H(q) for q in q0]))
    qg, pg, it, _ = ctx.leapfrog(P, q0, p0, 100, return_info=True)
    for c in range(n):
        qo, po, NP, NQ = m.trajectory(q0[c], p0[c], 100, record=False)
        assert it[c, 0] == NP.sum() and it[c, 1] == NQ.sum()
        assert_state_close(qg[c], qo, 1e-9, "q")
        assert_state_close(pg[c], po, 1e-8, "p")


def test_c5_gradient_energy_vs_oracle(gpu_lib):
    """256x256, K=64 with prior (windowed kernel) against the full-image oracle."""
    capi = gpu_lib
    z = load_golden("traj_c5")
    par = R.params_from_npz(z)
    ctx = _ctx(capi, z)
    P = capi_params(capi, par)
    m = R.RefModel(z["D"], par)
    q, p = z["Q"][0, :2], z["P"][0, :2]
    g = ctx.gradient(P, q, kind=1)
    for c in range(2):
        want = m.dphidq(q[c])
        assert np.abs(g[c] - want).max() / (np.abs(want).max() + 1) < 1e-10
    V, T = ctx.energy(P, q, p, f_pos=True)
    for c in range(2):
        np.testing.assert_allclose(V[c], m.V(q[c], f_pos=True), rtol=1e-12)
        np.testing.assert_allclose(T[c], m.T(p[c], m.H(q[c])), rtol=1e-12)


def test_errors(gpu_lib):
    capi = gpu_lib
    z = load_golden("traj_c1")
    par = R.params_from_npz(z)
    with pytest.raises(capi.RhmcError):
        capi.Context(np.zeros((4, 6)))          # rows != cols
    ctx = _ctx(capi, z)
    P = capi_params(capi, par)
    with pytest.raises(capi.RhmcError):
        ctx.leapfrog(P, np.zeros((2, 3 * 1025)), np.zeros((2, 3 * 1025)), 1)   # K > 1024
    with pytest.raises((capi.RhmcError, ValueError)):
        ctx.gradient(P, np.zeros((2, 0)))                                # K = 0
    bad = capi_params(capi, par)
    bad.reserved = 1
    with pytest.raises(capi.RhmcError):
        ctx.leapfrog(bad, z["Q"][:, 0], z["P"][:, 0], 1)
    # zero chains and zero steps are no-ops
    q, p = ctx.leapfrog(P, z["Q"][:, 0], z["P"][:, 0], 0)
    assert np.array_equal(q, z["Q"][:, 0]) and np.array_equal(p, z["P"][:, 0])
