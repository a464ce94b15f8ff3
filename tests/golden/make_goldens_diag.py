#!/usr/bin/env python3
"""Generate tests/golden/rhmc_diag.npz from the REFERENCE's own
samplers.lightsource_gym.RHMC_random_diag (build container only; see
make_goldens.py for how the reference is loaded — nothing of its source is
kept).

Per scene the reference's sampler runs after np.random.seed(run seed), then
tests/rhmc_diag_ref.py from the same seed.  Asserted: A_chain is identical and
q_chain / E_chain (with save_traj also qs / Vs / Ts) agree to 1e-13 relative,
infinities in the same places.  Stored from rhmc_diag_ref: the chains, the
draws z, steps, lnu, every trajectory's end state and whether its last step
flipped, the MH test's dE; the image as integer counts.

Asserted for the reference alone; the run seed is nudged until all hold:
  * every iteration with finite dE >= 0 has |lnu + dE| >= 1e-3;
  * a replay on the recorded draws with the gradient scaled by 1 +- 1e-13
    leaves every decision unchanged and moves every trajectory's end state by
    at most 0.1 of the bar the GPU tests put on it, i.e. by 1e-11 (|value| +
    1): the bar then tests the arithmetic, not the conditioning;
  * in `wall` at least one step flips, at least one trajectory ends on a flip
    and at least one iteration is non-finite;
  * accepted and rejected iterations both occur somewhere in the set.

The archive is written with fixed member timestamps, so a rerun reproduces the
file byte for byte.

Usage:  python tests/golden/make_goldens_diag.py [--ref /root/reference]
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
import rhmc_diag_ref  # noqa: E402

K1 = [(19.5, 16.3, 15.6)]
# name, side, stars (mag, x, y), f_lim as a magnitude (None: 0), dt_global,
# np.random.seed of gen_mock_data, save_traj
SCENES = [
    ("k1", 32, K1, None, 1e-2, 3, False),
    ("k1fast", 32, K1, None, 0.2, 3, False),
    ("k3", 48, [(19., 12.3, 30.6), (20.5, 33.2, 14.4), (21., 25.5, 25.1)], None, 0.1, 5, False),
    ("wall", 32, [(21.5, 10.3, 20.6), (20., 22., 9.)], 21.7, 0.2, 7, False),
    ("traj", 32, K1, None, 1e-2, 3, True),
]
NITER = 40
STEPS_MIN, STEPS_MAX = 10, 50
N_TRAJ = 5              # iterations of `traj` whose qs / Vs / Ts are stored
MARGIN = 1e-3
SENS_BAR = 0.1 * 1e-10  # a tenth of the GPU tests' bar, relative to |value| + 1
RTOL = 1e-13


def close(a, b):
    a, b = np.asarray(a, dtype=float), np.asarray(b, dtype=float)
    fin = np.isfinite(b)
    return a.shape == b.shape and np.array_equal(a[~fin], b[~fin], equal_nan=True) \
        and np.allclose(a[fin], b[fin], rtol=RTOL, atol=0.)


def moved(a, b):
    """max |a - b| / (|b| + 1) over the finite entries; inf if the non-finite differ."""
    fin = np.isfinite(b)
    if not np.array_equal(np.isfinite(a), fin):
        return np.inf
    return float((np.abs(a[fin] - b[fin]) / (np.abs(b[fin]) + 1.)).max()) if fin.any() else 0.


def conditions(name, ref_args, q0, dt, f_lim, run):
    """None, or the text of the first condition that fails."""
    dE, lnu = run["dE"], run["lnu"]
    with np.errstate(invalid="ignore"):
        tested = np.isfinite(dE) & (dE >= 0)
        margin = np.abs(lnu + dE)
    if tested.any() and margin[tested].min() < MARGIN:
        return "margin %.3g" % margin[tested].min()
    worst = 0.
    for sG in (1 + 1e-13, 1 - 1e-13):
        r = rhmc_diag_ref.DiagRef(*ref_args, scale_G=sG)
        got = r.run(q0, NITER, dt, f_lim, z=run["z"], steps=run["steps"], lnu=run["lnu"])
        if not np.array_equal(got["A_chain"], run["A_chain"]):
            return "a 1e-13 change of the gradient changes a decision"
        worst = max(worst, moved(got["q_end"], run["q_end"]), moved(got["p_end"], run["p_end"]))
    if worst > SENS_BAR:
        return "a 1e-13 change of the gradient moves an end state by %.3g" % worst
    if name == "wall":
        r = rhmc_diag_ref.DiagRef(*ref_args)
        n_flip = 0
        for i in range(NITER):          # the trajectories again, counting flipped steps
            tr = r.traj(run["q_chain"][i], run["z"][i + 1] * np.sqrt(
                r.mass_matrix(run["q_chain"][i])), int(run["steps"][i]), dt, f_lim)[3]
            n_flip += int((tr[1:, 0::3] < f_lim).any(axis=1).sum())
        if n_flip < 1 or run["flipped_last"].sum() < 1 or np.isfinite(dE).all():
            return "wall: %d flipped steps, %d last-step flips, %d non-finite" % (
                n_flip, run["flipped_last"].sum(), (~np.isfinite(dE)).sum())
        print("  wall: %d flipped steps, %d last-step flips, %d non-finite iterations" % (
            n_flip, run["flipped_last"].sum(), (~np.isfinite(dE)).sum()))
    print("  %-6s %2d accepted %2d rejected, min margin %.3g, 1e-13 sensitivity %.3g" % (
        name, run["A_chain"].sum(), NITER - run["A_chain"].sum(),
        margin[tested].min() if tested.any() else np.inf, worst))
    return None


def run_scene(L, U, name, side, stars, mag_lim, dt, seed, save_traj):
    g = L.lightsource_gym()
    g.num_rows = g.num_cols = side
    q_true = np.array([[U.mag2flux(m) * g.flux_to_count, x, y] for m, x, y in stars])
    np.random.seed(seed)
    g.gen_mock_data(q_true)
    g.compute_factors()
    f_lim = 0. if mag_lim is None else U.mag2flux(mag_lim) * g.flux_to_count
    q_model_0 = q_true * np.array([1.03, 1., 1.]) + np.array([0., 0.2, -0.15])
    ref_args = (g.D, g.B_count, g.PSF_FWHM_pix, g.factor1)
    assert rhmc_diag_ref.factor1_of(side, side, g.PSF_FWHM_pix) == g.factor1
    for nudge in range(50):
        run_seed = seed + 100 + nudge
        np.random.seed(run_seed)
        with contextlib.redirect_stdout(io.StringIO()), np.errstate(all="ignore"):
            g.RHMC_random_diag(q_model_0.copy(), Niter=NITER, steps_min=STEPS_MIN,
                               steps_max=STEPS_MAX, f_lim=f_lim, dt_global=dt,
                               save_traj=save_traj)
        nxt_reference = np.random.random()
        np.random.seed(run_seed)
        mine = rhmc_diag_ref.DiagRef(*ref_args)
        run = mine.run(q_model_0.reshape(-1), NITER, dt, f_lim, STEPS_MIN, STEPS_MAX,
                       save_traj=save_traj)
        assert np.random.random() == nxt_reference
        assert np.array_equal(run["A_chain"], g.A_chain[0, :, 0]), name
        assert close(run["q_chain"], g.q_chain[0]), name
        assert close(run["E_chain"], g.E_chain[0, :, 0]), name
        assert close(run["dE_chain"][np.isfinite(run["dE_chain"])],
                     g.dE_chain[0, :, 0][np.isfinite(run["dE_chain"])]), name
        if save_traj:
            for k in ("qs", "Vs", "Ts"):
                theirs = getattr(g, k)
                assert len(theirs) == len(run[k]) == NITER + 1
                for a, b in zip(run[k], theirs):
                    assert close(a, b), (name, k)
        why = conditions(name, ref_args, q_model_0.reshape(-1), dt, f_lim, run)
        if why is None:
            break
        print("  %s: run seed %d dropped (%s)" % (name, run_seed, why))
    else:
        raise AssertionError("no run seed for scene " + name)
    out = dict(D=as_counts(g.D), q_true=q_true, q_model_0=q_model_0, side=side, seed=seed,
               run_seed=run_seed, B_count=g.B_count, fwhm_pix=g.PSF_FWHM_pix,
               flux_to_count=g.flux_to_count, factor1=g.factor1, f_lim=f_lim, dt_global=dt,
               n_iter=NITER, steps_min=STEPS_MIN, steps_max=STEPS_MAX,
               next_random=nxt_reference, A_chain=run["A_chain"].astype(np.int8))
    assert np.array_equal(out["D"].astype(float), g.D)
    for k in ("q_chain", "E_chain", "dE_chain", "z", "steps", "lnu", "q_end", "p_end",
              "flipped_last", "dE"):
        out[k] = run[k]
    if save_traj:           # entry 0 (the start) and the first N_TRAJ iterations, NaN-padded
        n = [len(v) for v in run["Vs"][:N_TRAJ + 1]]
        out["traj_len"] = np.array(n, np.int32)
        qs = np.full((N_TRAJ + 1, max(n), q_model_0.size), np.nan)
        Vs = np.full((N_TRAJ + 1, max(n)), np.nan)
        Ts = np.full((N_TRAJ + 1, max(n)), np.nan)
        for i in range(N_TRAJ + 1):
            qs[i, :n[i]], Vs[i, :n[i]], Ts[i, :n[i]] = run["qs"][i], run["Vs"][i], run["Ts"][i]
        out.update(qs=qs, Vs=Vs, Ts=Ts)
    return {name + "/" + k: np.asarray(v) for k, v in out.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ref", default="/root/reference")
    ap.add_argument("--out", default=os.path.join(HERE, "rhmc_diag.npz"))
    args = ap.parse_args()
    S, U, L, tmp = load_reference(args.ref)
    try:
        out = {}
        for scene in SCENES:
            out.update(run_scene(L, U, *scene))
        A = np.concatenate([out[s[0] + "/A_chain"] for s in SCENES])
        assert A.any() and not A.all(), "accepted and rejected iterations must both occur"
        save_deterministic(args.out, out)
        print("wrote %s (%d bytes)" % (args.out, os.path.getsize(args.out)))
        assert os.path.getsize(args.out) < 256 * 1024
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


if __name__ == "__main__":
    main()
