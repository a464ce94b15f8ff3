#!/usr/bin/env python3
"""Generate tests/golden/rhmc_hess.npz from the REFERENCE's own
samplers.lightsource_gym.RHMC_random and RHMC_efficient_computation (build
container only; see make_goldens.py for how the reference is loaded — nothing
of its source is kept).

Per scene the reference's sampler runs after np.random.seed(run seed), then
tests/rhmc_hess_ref.py from the same seed.  Asserted: A_chain is identical,
q_chain / E_chain / dE_chain agree to 1e-13 relative with the non-finite
entries in the same places, the caller's array ends equal to the last row, and
the next random() is the same.  Stored from rhmc_hess_ref: the chains, the
draws z, steps, lnu, every trajectory's end state, steps_done and status word,
the MH test's dE, the printed lines; the image as integer counts.

Asserted for the reference alone; the run seed is nudged until all hold:
  * every iteration with finite dE >= 0 has |lnu + dE| >= 1e-3;
  * a replay on the recorded draws with the three derivative arrays scaled by
    1 +- 1e-13 leaves every decision, every steps_done and every status word
    unchanged and moves every trajectory's end state by at most 0.1 of the bar
    the GPU tests put on it, i.e. by 1e-11 (|value| + 1);
  * in `wall` at least one trajectory breaks off after a crossing in
    mid-trajectory and at least one dE is non-finite;
  * `stop` stops at i = 100 (R_accept < 50, samplers.py:1098-1101);
  * accepted and rejected iterations both occur somewhere in the set.

`fn1`, `fn3`, `fn10`: RHMC_efficient_computation recorded from the reference at
a handful of states for K = 1, 3, 10, both return forms, the last state below
the wall; asserted against the restatement to 1e-13.

The archive is written with fixed member timestamps, so a rerun reproduces the
file byte for byte.

Usage:  python tests/golden/make_goldens_hess.py [--ref /root/reference]
"""
import argparse
import contextlib
import io
import os
import shutil
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

from make_goldens import load_reference  # noqa: E402
from make_goldens_dt import as_counts, save_deterministic  # noqa: E402
from make_goldens_diag import close, moved  # noqa: E402
import rhmc_hess_ref  # noqa: E402

K1 = [(19.5, 16.3, 15.6)]
K3 = [(19., 12.3, 30.6), (20.5, 33.2, 14.4), (21., 25.5, 25.1)]
WALL = [(21.5, 10.3, 20.6), (20., 22., 9.)]
# name, side, stars (mag, x, y), f_lim as a magnitude (None: 0), dt_f, dt_xy,
# np.random.seed of gen_mock_data, Niter
SCENES = [
    ("k1", 32, K1, None, 0.1, 1.0, 3, 30),
    ("k1slow", 32, K1, None, 0.01, 0.1, 3, 30),
    ("k3", 48, K3, None, 0.1, 0.3, 5, 30),
    ("wall", 32, WALL, 22.2, 0.1, 0.3, 7, 30),
    ("stop", 32, WALL, 21.7, 0.3, 0.3, 7, 120),
]
K10 = [(19.0, 8.2, 9.7), (19.6, 14.5, 36.1), (20.1, 24.3, 22.8), (20.4, 39.6, 11.2),
       (20.8, 33.1, 40.4), (21.0, 6.7, 27.9), (21.2, 42.2, 29.5), (20.6, 18.9, 6.3),
       (19.9, 28.8, 33.6), (21.4, 37.4, 19.1)]
# name, side, stars, seed of gen_mock_data, f_lim as a magnitude
FUNCTIONS = [("fn1", 32, K1, 3, 22.2), ("fn3", 48, K3, 5, 22.2), ("fn10", 48, K10, 11, 22.5)]
N_STATES = 4            # per K; the last is below the wall
STEPS_MIN, STEPS_MAX = 10, 50
MARGIN = 1e-3
SENS_BAR = 0.1 * 1e-10  # a tenth of the GPU tests' bar, relative to |value| + 1


def gym_of(L, U, side, stars, seed):
    g = L.lightsource_gym()
    g.num_rows = g.num_cols = side
    q_true = np.array([[U.mag2flux(m) * g.flux_to_count, x, y] for m, x, y in stars])
    np.random.seed(seed)
    g.gen_mock_data(q_true)
    return g, q_true


def conditions(name, ref_args, q0, niter, dt_f, dt_xy, f_lim, run):
    """None, or the text of the first condition that fails."""
    n = run["n_run"]
    dE, lnu = run["dE"][:n], run["lnu"][:n]
    with np.errstate(invalid="ignore"):
        tested = np.isfinite(dE) & (dE >= 0)
        margin = np.abs(lnu + dE)
    if tested.any() and margin[tested].min() < MARGIN:
        return "margin %.3g" % margin[tested].min()
    worst = 0.
    for sG in (1 + 1e-13, 1 - 1e-13):
        r = rhmc_hess_ref.HessRef(*ref_args, scale_G=sG)
        got = r.run(q0.copy(), niter, dt_f, dt_xy, f_lim, z=run["z"], steps=run["steps"],
                    lnu=run["lnu"])
        for k in ("A_chain", "steps_done", "status"):
            if not np.array_equal(got[k], run[k]):
                return "a 1e-13 change of the derivatives changes " + k
        worst = max(worst, moved(got["q_end"], run["q_end"]), moved(got["p_end"], run["p_end"]))
    if worst > SENS_BAR:
        return "a 1e-13 change of the derivatives moves an end state by %.3g" % worst
    broke = (run["steps_done"][:n] < run["steps"][:n]) & (run["steps_done"][:n] > 0)
    if name == "wall":
        if broke.sum() < 1 or np.isfinite(dE).all():
            return "wall: %d broken trajectories, %d non-finite dE" % (
                broke.sum(), (~np.isfinite(dE)).sum())
    if name == "stop" and n != 100:
        return "stop: ran %d iterations" % n
    print("  %-6s %3d accepted %3d rejected of %3d, %2d broken off, %2d non-finite dE, "
          "min margin %.3g, 1e-13 sensitivity %.3g"
          % (name, run["A_chain"][:n].sum(), n - run["A_chain"][:n].sum(), n, broke.sum(),
             (~np.isfinite(dE)).sum(), margin[tested].min() if tested.any() else np.inf, worst))
    return None


def run_scene(L, U, name, side, stars, mag_lim, dt_f, dt_xy, seed, niter):
    g, q_true = gym_of(L, U, side, stars, seed)
    f_lim = 0. if mag_lim is None else U.mag2flux(mag_lim) * g.flux_to_count
    q_model_0 = q_true * np.array([1.03, 1., 1.]) + np.array([0., 0.2, -0.15])
    ref_args = (g.D, g.B_count, g.PSF_FWHM_pix)
    for nudge in range(50):
        run_seed = seed + 100 + nudge
        np.random.seed(run_seed)
        theirs_q0 = q_model_0.copy()
        printed = io.StringIO()
        with contextlib.redirect_stdout(printed), np.errstate(all="ignore"):
            g.RHMC_random(theirs_q0, Niter=niter, steps_min=STEPS_MIN, steps_max=STEPS_MAX,
                          f_lim=f_lim, dt_RHMC_xy=dt_xy, dt_RHMC_f=dt_f, debug=False)
        nxt_reference = np.random.random()
        np.random.seed(run_seed)
        mine = rhmc_hess_ref.HessRef(*ref_args)
        mine_q0 = q_model_0.copy()
        run = mine.run(mine_q0, niter, dt_f, dt_xy, f_lim, STEPS_MIN, STEPS_MAX)
        assert np.random.random() == nxt_reference
        assert np.array_equal(run["A_chain"], g.A_chain[0, :, 0]), name
        assert close(run["q_chain"], g.q_chain[0]), name
        assert close(run["E_chain"], g.E_chain[0, :, 0]), name
        assert close(run["dE_chain"], g.dE_chain[0, :, 0]), name
        assert printed.getvalue().splitlines() == run["lines"], name
        n = run["n_run"]
        assert np.array_equal(theirs_q0.reshape(-1), g.q_chain[0, n], equal_nan=True), name
        assert np.array_equal(mine_q0.reshape(-1), run["q_chain"][n], equal_nan=True), name
        assert not run["q_chain"][n + 1:].any() and not g.q_chain[0, n + 1:].any(), name
        why = conditions(name, ref_args, q_model_0, niter, dt_f, dt_xy, f_lim, run)
        if why is None:
            break
        print("  %s: run seed %d dropped (%s)" % (name, run_seed, why))
    else:
        raise AssertionError("no run seed for scene " + name)
    out = dict(D=as_counts(g.D), q_true=q_true, q_model_0=q_model_0, side=side, seed=seed,
               run_seed=run_seed, B_count=g.B_count, fwhm_pix=g.PSF_FWHM_pix,
               flux_to_count=g.flux_to_count, f_lim=f_lim, dt_f=dt_f, dt_xy=dt_xy,
               n_iter=niter, steps_min=STEPS_MIN, steps_max=STEPS_MAX,
               next_random=nxt_reference, A_chain=run["A_chain"].astype(np.int8),
               lines=np.array(run["lines"]))
    assert np.array_equal(out["D"].astype(float), g.D)
    for k in ("q_chain", "E_chain", "dE_chain", "z", "steps", "lnu", "q_end", "p_end",
              "steps_done", "status", "dE", "n_run"):
        out[k] = run[k]
    return {name + "/" + k: np.asarray(v) for k, v in out.items()}


def run_functions(L, U, name, side, stars, seed, mag_lim):
    g, q_true = gym_of(L, U, side, stars, seed)
    g.Nobjs = len(stars)
    g.d = 3 * g.Nobjs
    g.f_lim = f_lim = U.mag2flux(mag_lim) * g.flux_to_count
    rng = np.random.RandomState(1000 + seed)
    mine = rhmc_hess_ref.HessRef(g.D, g.B_count, g.PSF_FWHM_pix)
    q, p, dVdqq, dqdt, dpdt, E = [], [], [], [], [], []
    for s in range(N_STATES):
        qs = (q_true * (1. + 0.05 * rng.randn(g.Nobjs, 1) * np.array([1., 0., 0.]))
              + 0.3 * rng.randn(g.Nobjs, 3) * np.array([0., 1., 1.])).reshape(-1)
        if s == N_STATES - 1:
            qs[3 * (g.Nobjs - 1)] = 0.5 * f_lim
        assert (qs[0::3] >= f_lim).all() == (s < N_STATES - 1)
        ps = rng.randn(g.d) * np.sqrt(np.abs(mine.derivs(qs)[1]))
        with np.errstate(all="ignore"):
            h = g.RHMC_efficient_computation(qs.copy(), ps.copy(), debug=False, dVdqq_only=True)
            a, b, c = g.RHMC_efficient_computation(qs.copy(), ps.copy(), debug=False)
        assert close(mine.compute(qs, ps, f_lim, dVdqq_only=True), h), name
        ma, mb, mc = mine.compute(qs, ps, f_lim)
        if s == N_STATES - 1:
            assert a == b == c == np.inf and ma == mb == mc == np.inf
            a = b = np.full(g.d, np.inf)
        else:
            assert close(ma, a) and close(mb, b) and close(mc, c), name
        q.append(qs), p.append(ps), dVdqq.append(h), dqdt.append(a), dpdt.append(b), E.append(c)
    out = dict(D=as_counts(g.D), side=side, B_count=g.B_count, fwhm_pix=g.PSF_FWHM_pix,
               f_lim=f_lim, q=q, p=p, dVdqq=dVdqq, dqdt=dqdt, dpdt=dpdt, E=E)
    print("  %-6s %d states recorded" % (name, N_STATES))
    return {name + "/" + k: np.asarray(v) for k, v in out.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ref", default="/root/reference")
    ap.add_argument("--out", default=os.path.join(HERE, "rhmc_hess.npz"))
    args = ap.parse_args()
    S, U, L, tmp = load_reference(args.ref)
    try:
        out = {}
        for scene in SCENES:
            out.update(run_scene(L, U, *scene))
        for fn in FUNCTIONS:
            out.update(run_functions(L, U, *fn))
        A = np.concatenate([out[s[0] + "/A_chain"][:int(out[s[0] + "/n_run"])] for s in SCENES])
        assert A.any() and not A.all(), "accepted and rejected iterations must both occur"
        save_deterministic(args.out, out)
        print("wrote %s (%d bytes)" % (args.out, os.path.getsize(args.out)))
        assert os.path.getsize(args.out) < 256 * 1024
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


if __name__ == "__main__":
    main()
