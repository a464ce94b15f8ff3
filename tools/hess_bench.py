#!/usr/bin/env python3
"""Rates of RHMC_random's trajectories (rhmc_hess_random_device) beside
HMC_random's (rhmc_hmc_random_device) forced to RHMC_KERNEL_GENERIC, the other
one-wave-per-chain kernel with the whole image in LDS, on the same build,
shapes and inputs, for scale.

Chain-steps per second (leapfrog steps; one pass over the image for the three
derivative sets, or one gradient pass, each) at 30 steps per chain for K = 1, 3
and 10 on 48 px, 4,096 chains each.  The fields are Poisson images of magnitude
19.5-21.3 stars; every chain starts near the truth with a momentum drawn under
its metric, p = z sqrt|dVdqq|, and the steps dt_f = 0.1, dt_xy = 0.3 of the
fixture's scenes.  HMC_random gets the same q, p and steps and the
per-coordinate step vector dt / |dVdqq| at the truth.  One timed window is
--calls calls of the device entry point queued back to back on one stream, each
on its own copy of q and p, between two HIP events; the copies are restored
between windows.

Every shape is warmed up by a window first; the figure is the median of
--repeats windows and `times` holds them all.  Each measurement runs in a
child process of its own under --limit seconds; the first one that fails or
runs out of time ends the run.  One JSON line per measurement, and after each
shape's pair one line with the ratio hess / hmc_random_generic.

  python tools/hess_bench.py
  python tools/hess_bench.py --one hess 10 48 4096
"""
import argparse
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "hmc-stellar-toy-model_amd"))

SHAPES = [(1, 48, 4096), (3, 48, 4096), (10, 48, 4096)]
STEPS = 30
DT_F, DT_XY = 0.1, 0.3


def field(K, side, n):
    from rhmc_amd.photometry import gauss_PSF, mag2flux
    from rhmc_amd.samplers import lightsource_gym
    g = lightsource_gym()
    g.num_rows = g.num_cols = side
    rng = np.random.RandomState(1000 + K)
    mags = rng.uniform(19.5, 21.3, K)
    q_true = np.stack([mag2flux(mags) * g.flux_to_count, rng.uniform(5, side - 5, K),
                       rng.uniform(5, side - 5, K)], axis=1)
    lam = np.ones((side, side)) * g.B_count
    for f, x, y in q_true:
        lam += f * gauss_PSF(side, side, x, y, FWHM=g.PSF_FWHM_pix)
    g.D = rng.poisson(lam).astype(float)
    q0 = np.tile(q_true.reshape(-1), (n, 1))
    q0[:, 0::3] *= np.exp(0.03 * rng.randn(n, K))
    q0[:, 1::3] += 0.2 * rng.randn(n, K)
    q0[:, 2::3] += 0.2 * rng.randn(n, K)
    ctx, P = g._context(), g._params()
    p0 = rng.randn(n, 3 * K) * np.sqrt(np.abs(ctx.hess_derivs(P, q0)[1]))
    dtv = np.array([DT_F, DT_XY, DT_XY] * K) / np.abs(ctx.hess_derivs(P, q_true.reshape(-1))[1])
    return g, q0, p0, dtv


def run(which, K, side, n, repeats, calls):
    import torch
    g, q0, p0, dtv = field(K, side, n)
    ctx, P = g._context(), g._params()
    if which != "hess":
        ctx.set_kernel("generic")
    dev = torch.device("cuda:0")
    stream = torch.cuda.Stream()
    q_in, p_in = torch.from_numpy(q0).to(dev), torch.from_numpy(p0).to(dev)
    q = torch.empty((calls,) + tuple(q_in.shape), dtype=q_in.dtype, device=dev)
    p = torch.empty_like(q)
    steps = torch.full((n,), STEPS, dtype=torch.int32, device=dev)
    st = torch.zeros(n, dtype=torch.int32, device=dev)
    done = torch.zeros(n, dtype=torch.int32, device=dev)
    d_dt = torch.from_numpy(np.ascontiguousarray(dtv)).to(dev)
    times = []
    for r in range(repeats + 1):          # the first window warms up
        q.copy_(q_in.expand_as(q))
        p.copy_(p_in.expand_as(p))
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        with torch.cuda.stream(stream):
            e0.record(stream)
            for i in range(calls):
                if which == "hess":
                    ctx.hess_random_device(P, DT_F, DT_XY, q[i].data_ptr(), p[i].data_ptr(),
                                           steps.data_ptr(), n, K, status_ptr=st.data_ptr(),
                                           steps_done_ptr=done.data_ptr(),
                                           stream=stream.cuda_stream)
                else:
                    ctx.hmc_random_device(P, d_dt.data_ptr(), q[i].data_ptr(), p[i].data_ptr(),
                                          steps.data_ptr(), n, K, status_ptr=st.data_ptr(),
                                          stream=stream.cuda_stream)
            e1.record(stream)
        stream.synchronize()
        if r:
            times.append(e0.elapsed_time(e1) * 1e-3)
    status = st.cpu().numpy()
    t = float(np.median(times))
    out = dict(kind=which, K=K, side=side, chains=n, steps=STEPS, calls=calls, seconds=t,
               chain_steps_per_s=calls * n * STEPS / t, times=times,
               nonfinite=int((status & 1).sum()))
    if which == "hess":     # a trajectory that broke off did fewer steps than it is counted for
        out["broken_off"] = int((done.cpu().numpy() < STEPS).sum())
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--one", nargs=4, help="hess|hmc_random_generic K SIDE CHAINS")
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--calls", type=int, default=10, help="calls per timed window")
    ap.add_argument("--limit", type=int, default=120, help="seconds per measurement")
    a = ap.parse_args()
    if a.one:
        print(json.dumps(run(a.one[0], int(a.one[1]), int(a.one[2]), int(a.one[3]), a.repeats,
                             a.calls)), flush=True)
        return 0
    for K, side, n in SHAPES:
        rate = {}
        for which in ("hess", "hmc_random_generic"):
            job = [which, str(K), str(side), str(n)]
            try:
                r = subprocess.run([sys.executable, os.path.abspath(__file__), "--one"] + job +
                                   ["--repeats", str(a.repeats), "--calls", str(a.calls)],
                                   timeout=a.limit,
                                   capture_output=True, text=True)
                rc, out = r.returncode, r.stdout
                sys.stderr.write(r.stderr)
            except subprocess.TimeoutExpired:
                rc, out = 124, ""
            if rc != 0:
                print("hess_bench: %s ended with status %d; stopping" % (" ".join(job), rc),
                      file=sys.stderr)
                return 1
            sys.stdout.write(out)
            sys.stdout.flush()
            rate[which] = json.loads(out.strip().splitlines()[-1])["chain_steps_per_s"]
        print(json.dumps(dict(kind="ratio", K=K, side=side, chains=n,
                              hess_over_hmc_random_generic=rate["hess"]
                              / rate["hmc_random_generic"])),
              flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
