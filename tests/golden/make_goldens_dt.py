#!/usr/bin/env python3
"""Generate tests/golden/find_best_dt.npz from the REFERENCE's own
samplers.lightsource_gym.HMC_find_best_dt (build container only; see
make_goldens.py for how the reference is loaded — nothing of its source is
kept).

Per scene the reference's search (default=False) runs after
np.random.seed(seed + 100), then tests/dt_ref.py from the same seed.  Asserted:
the final dt is bit-identical, and every E_single value the reference evaluated
(its instance's E_single is wrapped, the way make_goldens_peaks.Recorder wraps
V_single) equals dt_ref's to 1e-13.  Stored from dt_ref: per trial star, phase,
stage, dt and A_rate; per iteration the draws z, steps, lnu and dE, accept and
q after the iteration (the margin |lnu + dE| follows from them); the Poisson
realisation of every star (integers; the tests rebuild M = realisation -
f0 PSF); the reference's dt and the next np.random.random() after its search.
One grad="full" search per scene is stored the same way under "<scene>/full/":
dt_ref only, the reference has no such mode.

Asserted for the reference alone (both searches of a scene):
  * every iteration with finite dE >= 0 has |lnu + dE| >= 1e-3 (the full
    search's seed is nudged until every condition holds);
  * a rerun with the gradient scaled by 1 +- 1e-11 and V by 1 +- 1e-12 leaves
    every decision and the final dt unchanged;
  * every trial replayed on its recorded draws with the gradient scaled by
    1 +- 1e-13 moves the dE of an iteration compared in value by at most a
    tenth of the bar the GPU tests put on it, 2e-10 |V(q0)| + 1e-9 |dE| (so
    that the bar tests the arithmetic, not the conditioning of a trajectory:
    the reference's searches stay below 2e-4 of it, a grad="full" search can
    hold chaotic trajectories with a small |dE| that exceed it 300-fold);
  * accepted, finite-rejected and non-finite iterations all occur;
  * at least 60 % of the iterations are compared in value (finite |dE| <= 50).

The archive is written with fixed member timestamps, so a rerun reproduces the
file byte for byte.

Usage:  python tests/golden/make_goldens_dt.py [--ref /root/reference]
"""
import argparse
import contextlib
import io
import os
import shutil
import sys
import zipfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

from make_goldens import load_reference  # noqa: E402
import dt_ref  # noqa: E402

# name, side, stars (mag, x, y), np.random.seed of gen_mock_data
SCENES = [
    ("A", 32, [(19.5, 10.3, 20.6), (20.5, 22.2, 9.4)], 3),
    ("B", 48, [(19., 12.3, 30.6), (20.5, 33.2, 14.4), (21., 25.5, 25.1)], 5),
    ("C", 32, [(17., 16.3, 15.6), (21.5, 5.2, 25.4)], 11),
    ("D", 64, [(18.5, 40.5, 45.1), (20., 12.3, 30.6)], 7),
    ("E", 40, [(20., 20.4, 18.7)], 13),
    ("F", 16, [(19.5, 8.3, 7.6)], 17),
]
N_ITER = 10
MARGIN = 1e-3
SENSITIVITY = 0.1
COMPARED_DE = 50.


def compared(dE):
    with np.errstate(invalid="ignore"):
        return np.isfinite(dE) & (np.abs(dE) <= COMPARED_DE)


def run_ref_search(ref, gym, q_model_0, seed, grad, scale_G=1., scale_V=1.):
    """dt_ref's search from np.random.seed(seed): (dt, trial log, realisations,
    E_single values, the next random())."""
    r = dt_ref.DtRef(ref.D, ref.fwhm, scale_G, scale_V)
    r.E_log = []
    reals = []

    def gen_mock():
        d = gym.gen_mock_data(q_model_0, return_data=True)
        reals.append(d.copy())
        return d

    np.random.seed(seed)
    log = []
    dt = dt_ref.search(r, q_model_0, gen_mock, Niter_per_trial=N_ITER, grad=grad, log=log)
    return dt, log, np.array(reals), np.array(r.E_log), np.random.random()


def sensitivity(ref, q_model_0, log, grad):
    """The largest change of a compared iteration's dE, in units of the GPU
    tests' bar on it, when its trial is replayed on the recorded draws with the
    gradient scaled by 1 +- 1e-13 (inf if a decision changes)."""
    M, V0 = {}, {}
    for t in log:                       # the backgrounds, from the log's own first V
        M.setdefault(t["star"], t["M"])
    base = dt_ref.DtRef(ref.D, ref.fwhm)
    for l in M:
        V0[l] = abs(base.V(q_model_0[l], M[l]))
    worst = 0.
    for sG in (1 + 1e-13, 1 - 1e-13):
        r = dt_ref.DtRef(ref.D, ref.fwhm, scale_G=sG)
        for t in log:
            got = r.trial(q_model_0[t["star"]], t["dt"], M[t["star"]], len(t["dE"]),
                          t["phase"] == dt_ref.FLUX, grad, z=t["z"], steps=t["steps"],
                          lnu=t["lnu"])
            if not np.array_equal(got["accept"], t["accept"]):
                return np.inf
            c = compared(t["dE"])
            if c.any():
                bar = 2e-10 * V0[t["star"]] + 1e-9 * np.abs(t["dE"][c])
                worst = max(worst, (np.abs(got["dE"][c] - t["dE"][c]) / bar).max())
    return worst


def decisions(log):
    return np.array([t["accept"] for t in log])


def conditions(name, ref, gym, q_model_0, seed, grad, dt, log):
    """The four conditions; returns None or the text of the first that fails."""
    dE = np.array([t["dE"] for t in log])
    lnu = np.array([t["lnu"] for t in log])
    acc = decisions(log).astype(bool)
    fin = np.isfinite(dE)
    with np.errstate(invalid="ignore"):
        tested = fin & (dE >= 0)
        margin = np.abs(lnu + dE)
    if tested.any() and margin[tested].min() < MARGIN:
        return "margin %.3g" % margin[tested].min()
    if not (acc.any() and (fin & ~acc).any() and (~fin).any()):
        return "kinds of iterations"
    if compared(dE).mean() < 0.6:
        return "compared in value %.2f" % compared(dE).mean()
    sens = sensitivity(ref, q_model_0, log, grad)
    if sens > SENSITIVITY:
        return "a 1e-13 change of the gradient moves dE by %.3g of its bar" % sens
    for sG, sV in ((1 + 1e-11, 1 + 1e-12), (1 - 1e-11, 1 - 1e-12), (1 + 1e-11, 1 - 1e-12),
                   (1 - 1e-11, 1 + 1e-12)):
        dt2, log2, _, _, _ = run_ref_search(ref, gym, q_model_0, seed, grad, sG, sV)
        if len(log2) != len(log) or not np.array_equal(decisions(log2), decisions(log)) \
                or not np.array_equal(dt2, dt):
            return "not robust to scaling"
    print("  %s %-9s %2d trials %3d iterations: %3d accepted %3d rejected %3d non-finite, "
          "%.0f%% compared, min margin %.3g, 1e-13 sensitivity %.3g of the bar" % (
              name, grad, len(log), dE.size, acc.sum(), (fin & ~acc).sum(), (~fin).sum(),
              100 * compared(dE).mean(), margin[tested].min() if tested.any() else np.inf, sens))
    return None


def as_counts(a):
    """Poisson counts as the smallest unsigned integer type that holds them."""
    assert np.array_equal(a, np.round(a)) and a.min() >= 0 and a.max() < 2 ** 32
    return a.astype(np.uint16 if a.max() < 65536 else np.uint32)


def pack_search(prefix, q_model_0, dt, log, reals, nxt, seed):
    return {
        prefix + "search_seed": np.asarray(seed),
        prefix + "dt": dt,
        prefix + "next_random": np.asarray(nxt),
        prefix + "realisations": as_counts(reals),
        prefix + "star": np.array([t["star"] for t in log], np.int32),
        prefix + "phase": np.array([t["phase"] for t in log], np.int32),
        prefix + "stage": np.array([t["stage"] for t in log], np.int32),
        prefix + "trial_dt": np.array([t["dt"] for t in log]),
        prefix + "A_rate": np.array([t["A_rate"] for t in log]),
        prefix + "z": np.array([t["z"] for t in log]),
        prefix + "steps": np.array([t["steps"] for t in log], np.int32),
        prefix + "lnu": np.array([t["lnu"] for t in log]),
        prefix + "dE": np.array([t["dE"] for t in log]),
        prefix + "accept": np.array([t["accept"] for t in log], np.int8),
        prefix + "q": np.array([t["q"] for t in log]),
    }


def run_scene(L, U, name, side, stars, seed):
    g = L.lightsource_gym()
    g.num_rows = g.num_cols = side
    q_true = np.array([[U.mag2flux(m) * g.flux_to_count, x, y] for m, x, y in stars])
    np.random.seed(seed)
    g.gen_mock_data(q_true)
    q_model_0 = q_true * np.array([1.03, 1., 1.]) + np.array([0., 0.2, -0.15])
    # the reference's own search, its E_single wrapped
    E_ref = []
    orig_E = g.E_single

    def E_single(q_single, p_single, model_data):
        e = orig_E(q_single, p_single, model_data)
        E_ref.append(float(e))
        return e

    g.E_single = E_single
    np.random.seed(seed + 100)
    with contextlib.redirect_stdout(io.StringIO()), np.errstate(all="ignore"):
        g.HMC_find_best_dt(q_model_0, Niter_per_trial=N_ITER)
    dt_reference = np.array(g.dt, dtype=float)
    nxt_reference = np.random.random()
    g.E_single = orig_E
    # dt_ref from the same seed
    ref = dt_ref.DtRef(g.D, g.PSF_FWHM_pix)
    dt, log, reals, E_mine, nxt = run_ref_search(ref, g, q_model_0, seed + 100, "reference")
    assert np.array_equal(dt, dt_reference), (name, dt, dt_reference)
    assert nxt == nxt_reference
    E_ref = np.array(E_ref)
    assert E_ref.shape == E_mine.shape, (E_ref.shape, E_mine.shape)
    both = np.isfinite(E_ref)
    assert np.array_equal(both, np.isfinite(E_mine))
    assert np.allclose(E_mine[both], E_ref[both], rtol=1e-13, atol=0.)
    n_it = sum(len(t["dE"]) for t in log)
    assert 110 <= n_it <= 400, (name, len(log), n_it)
    why = conditions(name, ref, g, q_model_0, seed + 100, "reference", dt, log)
    assert why is None, (name, why)
    out = {name + "/" + k: np.asarray(v) for k, v in dict(
        D=as_counts(g.D), q_true=q_true, q_model_0=q_model_0, side=side, seed=seed,
        B_count=g.B_count, fwhm_pix=g.PSF_FWHM_pix, flux_to_count=g.flux_to_count,
        n_iter=N_ITER).items()}
    assert np.array_equal(out[name + "/D"].astype(float), g.D)
    out.update(pack_search(name + "/", q_model_0, dt, log, reals, nxt, seed + 100))
    # one grad="full" search (dt_ref only), its seed nudged until the conditions hold
    for nudge in range(50):
        s_full = seed + 200 + nudge
        try:
            dtf, logf, realsf, _, nxtf = run_ref_search(ref, g, q_model_0, s_full, "full")
        except RuntimeError:
            continue
        why = conditions(name, ref, g, q_model_0, s_full, "full", dtf, logf)
        if why is None:
            break
        print("  %s full: seed %d dropped (%s)" % (name, s_full, why))
    else:
        raise AssertionError("no seed for the full search of " + name)
    out.update(pack_search(name + "/full/", q_model_0, dtf, logf, realsf, nxtf, s_full))
    print("%s: reference dt %s, full dt %s" % (name, dt, dtf))
    return out


def save_deterministic(path, arrays):
    """np.savez_compressed with fixed member timestamps (np.load reads it)."""
    with zipfile.ZipFile(path, "w", zipfile.ZIP_DEFLATED) as zf:
        for key in sorted(arrays):
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.asanyarray(arrays[key]), allow_pickle=False)
            info = zipfile.ZipInfo(key + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            info.external_attr = 0o644 << 16
            zf.writestr(info, buf.getvalue(), compresslevel=9)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ref", default="/root/reference")
    ap.add_argument("--out", default=os.path.join(HERE, "find_best_dt.npz"))
    args = ap.parse_args()
    S, U, L, tmp = load_reference(args.ref)
    try:
        out = {}
        for scene in SCENES:
            out.update(run_scene(L, U, *scene))
        save_deterministic(args.out, out)
        print("wrote %s (%d bytes)" % (args.out, os.path.getsize(args.out)))
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


if __name__ == "__main__":
    main()
