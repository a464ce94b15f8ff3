#!/usr/bin/env python3
"""Rates of HMC_find_best_dt's step-size search (rhmc_dt_trials).

1. Trial-steps per second (leapfrog steps, one gradient pass each) for n =
   1, 8, 64, 1,024 and 16,384 tasks with 64 and with 256 lanes per task
   (RHMC_OPT_DT_LANES), at 48 px (scene B of tests/golden/find_best_dt.npz,
   where the 64-lane kernel reads its pixels from global memory) and at 32 px
   (scene A, both register-resident).  The tasks are the scene's recorded
   fine-stage trials, repeated, with the device's Philox draws; the time is the
   HIP-event time of the device entry point on its stream.
2. Wall time of the whole search at 3 model stars (scene B) and at 64 (a
   64-px field of magnitude 19-21 stars): rng="numpy", rng="philox", and the
   NumPy restatement tests/dt_ref.py on the same box; a host clock around the
   call, which ends in a synchronise.

Every shape is warmed up first; the figure is the median of --repeats runs and
`times` holds them all.  Each measurement runs in a child process of its own
under --limit seconds; the first one that fails or runs out of time ends the
run.  One JSON line per measurement.

  python tools/dt_bench.py
  python tools/dt_bench.py --one rate 48 256 1024
  python tools/dt_bench.py --one search philox 64
"""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "hmc-stellar-toy-model_amd"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)


def scene(name):
    import dt_ref
    return dt_ref.load_scene(np.load(os.path.join(ROOT, "tests", "golden", "find_best_dt.npz")),
                             name)


def params(capi, s):
    return capi.make_params(dt=1., delta=1e-6, counter_max=1000, B_count=s["B_count"], f_lim=0.,
                            f_low=1., fwhm_pix=s["fwhm"], g_xx=1., g_ff=1., g_ff2=1., g0=1.,
                            g1=1., g2=1.)


def run_rate(side, lanes, n, repeats):
    import torch
    from rhmc_amd import capi
    s = scene({48: "B", 32: "A"}[side])
    rows = np.flatnonzero(s["stage"] == 1)
    rows = rows[np.arange(n) % len(rows)]
    ni = s["n_iter"]
    ctx = capi.Context(s["D"], device=0)
    ctx.set_option(capi.OPT_DT_LANES, lanes)
    P, opts = params(capi, s), capi.make_dt_opts(ni, "reference", 10, 50)
    dev = torch.device("cuda:0")
    stream = torch.cuda.Stream()

    def up(a, dtype):
        return torch.from_numpy(np.ascontiguousarray(a, dtype)).to(dev)

    bg, bgi = up(s["M"], np.float64), up(s["star"][rows], np.int32)
    q0, dt = up(s["q0"][rows], np.float64), up(s["dt"][rows], np.float64)
    fo = up(s["flux_only"][rows], np.int32)
    sid = up(np.arange(n), np.int64)
    steps = torch.zeros((n, ni), dtype=torch.int32, device=dev)
    n_acc = torch.zeros(n, dtype=torch.int32, device=dev)
    rec = capi.DtRecord(0, 0, 0, 0, steps.data_ptr(), 0)
    times = []
    for r in range(repeats + 1):          # the first call warms up
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        with torch.cuda.stream(stream):
            e0.record(stream)
            ctx.dt_trials_device(P, opts, bg.data_ptr(), len(s["M"]), bgi.data_ptr(),
                                 q0.data_ptr(), dt.data_ptr(), n, flux_only_ptr=fo.data_ptr(),
                                 seed=1, stream_id_ptr=sid.data_ptr(),
                                 n_accept_ptr=n_acc.data_ptr(), record=rec,
                                 stream=stream.cuda_stream)
            e1.record(stream)
        stream.synchronize()
        if r:
            times.append(e0.elapsed_time(e1) * 1e-3)
    total = int(steps.cpu().numpy().sum())
    acc = float(n_acc.cpu().numpy().mean() / ni)
    ctx.close()
    t = float(np.median(times))
    return dict(kind="rate", side=side, lanes=lanes, tasks=n, n_iter=ni, trial_steps=total,
                seconds=t, trial_steps_per_s=total / t, times=times, acceptance=acc)


def field(n_stars):
    """(side, q_true, q_model_0): scene B for 3 stars, else a 64-px field."""
    from rhmc_amd.photometry import default_exp_setup, mag2flux
    if n_stars == 3:
        s = scene("B")
        return s["side"], None, s["q_model_0"], s["D"], s["search_seed"]
    rs = np.random.RandomState(41)
    flux_to_count = default_exp_setup()[2]
    q = np.stack([mag2flux(rs.uniform(19., 21., n_stars)) * flux_to_count,
                  rs.uniform(4., 60., n_stars), rs.uniform(4., 60., n_stars)], axis=1)
    return 64, q, q * np.array([1.03, 1., 1.]) + np.array([0., 0.2, -0.15]), None, 141


def run_search(mode, n_stars, repeats):
    from rhmc_amd.samplers import lightsource_gym
    import dt_ref
    side, q_true, q_model_0, D, seed = field(n_stars)
    g = lightsource_gym()
    g.num_rows = g.num_cols = side
    if D is None:
        np.random.seed(40)
        g.gen_mock_data(q_true)
    else:
        g.D = D
    times, dts = [], []
    for r in range(repeats + 1):          # the first run warms up
        np.random.seed(seed)
        t0 = time.perf_counter()
        if mode == "dt_ref":
            ref = dt_ref.DtRef(g.D, g.PSF_FWHM_pix)
            dt = dt_ref.search(ref, q_model_0,
                               lambda: g.gen_mock_data(q_model_0, return_data=True))
        else:
            g.HMC_find_best_dt(q_model_0, rng=mode, seed=3)
            dt = g.dt.copy()
        t = time.perf_counter() - t0
        if r or mode == "dt_ref":         # (NumPy needs no warm-up; its first run counts)
            times.append(t)
        dts.append(dt)
        if mode == "dt_ref" and len(times) == repeats:
            break
    return dict(kind="search", mode=mode, stars=n_stars, side=side, seconds=float(np.median(times)),
                times=times, reproducible=bool(all(np.array_equal(d, dts[0]) for d in dts)),
                dt_f_median=float(np.median(dts[0][0::3])),
                dt_xy_median=float(np.median(dts[0][1::3])))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--one", nargs="+", help="rate SIDE LANES N | search MODE STARS")
    ap.add_argument("--sizes", type=int, nargs="+", default=[1, 8, 64, 1024, 16384])
    ap.add_argument("--sides", type=int, nargs="+", default=[48, 32])
    ap.add_argument("--stars", type=int, nargs="+", default=[3, 64])
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--cpu-repeats", type=int, default=2)
    ap.add_argument("--limit", type=int, default=300, help="seconds per measurement")
    a = ap.parse_args()
    if a.one:
        if a.one[0] == "rate":
            r = run_rate(int(a.one[1]), int(a.one[2]), int(a.one[3]), a.repeats)
        else:
            r = run_search(a.one[1], int(a.one[2]),
                           a.cpu_repeats if a.one[1] == "dt_ref" else a.repeats)
        print(json.dumps(r), flush=True)
        return 0
    jobs = [["rate", str(side), str(lanes), str(n)] for side in a.sides for n in a.sizes
            for lanes in (256, 64)]
    jobs += [["search", mode, str(k)] for k in a.stars for mode in ("numpy", "philox", "dt_ref")]
    for job in jobs:
        try:
            rc = subprocess.run([sys.executable, os.path.abspath(__file__), "--one"] + job +
                                ["--repeats", str(a.repeats), "--cpu-repeats",
                                 str(a.cpu_repeats)], timeout=a.limit).returncode
        except subprocess.TimeoutExpired:
            rc = 124
        if rc != 0:
            print("dt_bench: %s ended with status %d; stopping" % (" ".join(job), rc),
                  file=sys.stderr)
            return 1
    return 0


if __name__ == "__main__":
    sys.exit(main())
