#!/usr/bin/env python3
"""Generate tests/golden/find_peaks.npz from the REFERENCE's own
samplers.lightsource_gym.find_peaks (build container only; see make_goldens.py
for how the reference is loaded — nothing of its source is kept).

find_peaks returns only the merged seeds.  Everything else is recovered by
wrapping the instance's V_single / dVdq_single (the way make_goldens.Counter
recovers fixed-point counts): the calls of one seed are V, (dVdq, V)*, with a
trailing dVdq when the seed went faint (samplers.py:192-221), and a seed's
first V call is the one at its grid position.  From them: the per-seed step
count (dVdq calls), stop reason, final state (the last V call's argument; for
a faint seed the update :201-207 of its last dVdq call, same expressions) and
the last V evaluated.

Near-threshold noise.  The convergence test compares |dV/V| with 1e-9 and the
reference's ratio carries np.sum's rounding.  For every step whose ratio lies
within a factor 2 of the threshold the ratio is re-evaluated with math.fsum
(tests/peaks_ref.py, fsum=True) and the largest change, in units of the
threshold, is stored per case as `noise`; the tests exempt a seed from the
exact step-count rule only if its ratio came within 10 x that of the
threshold at some step (`ratio_margin`, per seed) or its flux within 1e-9
relative of f_lim (`f_margin`).  At most 5 % of a case's seeds may be exempt:
asserted here for the reference alone.

Usage:  python tests/golden/make_goldens_peaks.py [--ref /root/reference]
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

from make_goldens import load_reference, pack  # noqa: E402
import peaks_ref  # noqa: E402

REL_TOL = 1e-9
REASONS = {"converged": 0, "faint": 1, "cap": 2}

# name, side, linear_pix_density, stars (mag, x, y), np.random.seed, Nstep, expected seeds
CASES = [
    ("A", 32, 0.25, [(19.5, 10.3, 20.6), (20.5, 22.2, 9.4)], 3, 1000, 49),
    ("A60", 32, 0.25, [(19.5, 10.3, 20.6), (20.5, 22.2, 9.4)], 3, 60, 49),
    ("B", 48, 0.2, [(19., 12.3, 30.6), (20.5, 33.2, 14.4), (21., 25.5, 25.1)], 5, 1000, 64),
    ("C", 64, 0.2, [(19., 12.3, 30.6), (20.5, 50.2, 14.4), (18., 40.5, 45.1), (20., 1.2, 62.8)],
     7, 1000, 121),
]
# the stop reasons each case is meant to show
MUST_SHOW = {"A": {"faint", "converged", "cap"}, "A60": {"faint", "cap"},
             "B": {"faint", "converged", "cap"}, "C": {"faint", "converged"}}


class Recorder:
    """Wrap a gym's V_single / dVdq_single to log (kind, q, value) per call."""

    def __init__(self, gym):
        self.calls = []
        orig_V, orig_G = gym.V_single, gym.dVdq_single

        def V_single(q_single, model_data):
            v = orig_V(q_single, model_data)
            self.calls.append(("V", tuple(float(t) for t in q_single), float(v)))
            return v

        def dVdq_single(q_single, model_data, **kw):
            g = orig_G(q_single, model_data, **kw)
            self.calls.append(("G", tuple(float(t) for t in q_single),
                               tuple(float(t) for t in g)))
            return g

        gym.V_single = V_single
        gym.dVdq_single = dVdq_single


def make_gym(L, U, side, stars, seed):
    g = L.lightsource_gym()
    g.num_rows = g.num_cols = side
    q_true = np.array([[U.mag2flux(m) * g.flux_to_count, x, y] for m, x, y in stars])
    np.random.seed(seed)
    g.gen_mock_data(q_true)
    return g, q_true


def split_calls(calls, grid):
    """The call log cut per seed: seed idx starts at the V call at grid[idx]."""
    out, cur, nxt = [], None, 0
    for c in calls:
        if c[0] == "V" and nxt < len(grid) and c[1] == tuple(grid[nxt]):
            cur = []
            out.append(cur)
            nxt += 1
        cur.append(c)
    assert len(out) == len(grid), (len(out), len(grid))
    return out


def run_case(L, U, name, side, dens, stars, seed, nstep, nseeds):
    # the grid alone (no_perturb), then the same stream again for the full run
    g, q_true = make_gym(L, U, side, stars, seed)
    g.find_peaks(linear_pix_density=dens, Nstep=nstep, no_perturb=True)
    grid = g.q_seed.copy()
    assert grid.shape == (nseeds, 3), grid.shape
    g, q_true = make_gym(L, U, side, stars, seed)
    rec = Recorder(g)
    with contextlib.redirect_stdout(io.StringIO()):
        g.find_peaks(linear_pix_density=dens, Nstep=nstep)
    mag_lim = g.mB - 1.
    f_lim = U.mag2flux(mag_lim) * g.flux_to_count           # samplers.py:157-161
    ref = peaks_ref.PeaksRef(g.D, g.B_count, g.PSF_FWHM_pix)
    per = split_calls(rec.calls, grid)
    n = len(per)
    q_fin = np.zeros((n, 3))
    steps = np.zeros(n, np.int32)
    reason = np.zeros(n, np.int32)
    V_fin = np.zeros(n)
    ratio_margin = np.full(n, np.inf)
    f_margin = np.full(n, np.inf)
    noise = 0.0
    n_near = 0
    for i, calls in enumerate(per):
        Vs = [c for c in calls if c[0] == "V"]
        Gs = [c for c in calls if c[0] == "G"]
        assert Vs[0][1] == tuple(grid[i])
        steps[i] = len(Gs)
        V_fin[i] = Vs[-1][2]
        if calls[-1][0] == "G":                               # :209-211
            reason[i] = REASONS["faint"]
            (f, x, y), (gf, gx, gy) = calls[-1][1], calls[-1][2]
            dt_f = f * 1e-1
            dt_xy = 1e-1 / f
            f -= gf * dt_f
            x -= gx * dt_xy
            y -= gy * dt_xy
            assert f < f_lim
            q_fin[i] = (f, x, y)
        else:
            q_fin[i] = Vs[-1][1]
            r = np.abs((Vs[-1][2] - Vs[-2][2]) / Vs[-2][2])   # :215
            reason[i] = REASONS["converged"] if r < REL_TOL else REASONS["cap"]
            assert reason[i] == REASONS["converged"] or steps[i] == nstep
        for k in range(1, len(Vs)):
            r = np.abs((Vs[k][2] - Vs[k - 1][2]) / Vs[k - 1][2])
            ratio_margin[i] = min(ratio_margin[i], abs(r - REL_TOL) / REL_TOL)
            if REL_TOL / 2 < r < REL_TOL * 2:
                a = ref.V(*Vs[k - 1][1], fsum=True)
                b = ref.V(*Vs[k][1], fsum=True)
                noise = max(noise, abs(abs((b - a) / a) - r) / REL_TOL)
                n_near += 1
        fs = [c[1][0] for c in Vs[1:]] + ([q_fin[i, 0]] if calls[-1][0] == "G" else [])
        for f in fs:
            f_margin[i] = min(f_margin[i], abs(f - f_lim) / f_lim)
    survivors = q_fin[reason != REASONS["faint"]]
    names = {v: k for k, v in REASONS.items()}
    shown = {names[r] for r in reason}
    assert MUST_SHOW[name] <= shown, (name, shown)
    band = 10 * noise
    exempt = int(np.sum((ratio_margin < band) | (f_margin < 1e-9)))
    assert exempt <= 0.05 * n, (name, exempt, n)
    # peaks_ref restates the reference: same counts and reasons, states to 1e-13
    q2, s2, r2, V2 = ref.descend_all(grid, f_lim, n_step=nstep)
    assert np.array_equal(s2, steps) and [REASONS[r] for r in r2] == list(reason)
    assert np.allclose(q2, q_fin, rtol=1e-13, atol=1e-13)
    print("%-4s %3d seeds: %3d faint %3d converged %3d cap, steps %d-%d, %d near-threshold steps, "
          "noise %.3g of the threshold (band %.3g), closest ratio %.3g, closest f %.3g, "
          "%d exempt" % (name, n, np.sum(reason == 1), np.sum(reason == 0), np.sum(reason == 2),
                         steps.min(), steps.max(), n_near, noise, band, ratio_margin.min(),
                         f_margin.min(), exempt))
    return pack(name + "/", dict(
        D=g.D, q_true=q_true, side=side, density=dens, seed=seed, Nstep=nstep, f_lim=f_lim,
        f_seed=grid[0, 0], B_count=g.B_count, fwhm_pix=g.PSF_FWHM_pix,
        flux_to_count=g.flux_to_count, mB=g.mB, grid=grid, q_final=q_fin, steps=steps,
        reason=reason, V_final=V_fin, ratio_margin=ratio_margin, f_margin=f_margin,
        noise=noise, merge_in=survivors, merge_out=np.asarray(g.q_seed, dtype=float)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ref", default="/root/reference")
    args = ap.parse_args()
    S, U, L, tmp = load_reference(args.ref)
    try:
        out = {}
        for case in CASES:
            out.update(run_case(L, U, *case))
        # HMC_find_best_dt(default=True) on case B's merged seeds (samplers.py:283-303)
        g = L.lightsource_gym()
        g.q_seed = out["B/merge_out"]
        with contextlib.redirect_stdout(io.StringIO()):
            g.HMC_find_best_dt(default=True)
        out["B/dt_default"] = np.asarray(g.dt, dtype=float)
        np.savez_compressed(os.path.join(HERE, "find_peaks.npz"), **out)
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


if __name__ == "__main__":
    main()
