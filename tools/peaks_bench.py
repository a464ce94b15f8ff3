#!/usr/bin/env python3
"""Seed-descent-steps per second of rhmc_find_peaks at 48 px: the one-launch
kernel against the stepwise path, and the reference-order NumPy loop
(tests/peaks_ref.py) on the CPU.

Workload: case B's image of tests/golden/find_peaks.npz (48 px, three stars)
and N caller-supplied seeds on a jittered grid (N = 4,096 and 65,536), the
reference's defaults otherwise (Nstep 1000, coefficients 0.1, f_lim at
mB - 1).  The rate is sum(steps) / time: the HIP-event time on the launch
stream for the GPU (device entry point, one warm-up call first), wall time
for the CPU loop, which runs on the first --cpu-seeds seeds only.

  python tools/peaks_bench.py                 # every measurement, one child process each
  python tools/peaks_bench.py --one fused 4096
Each GPU measurement runs in a child process of its own under --limit seconds;
the first one that fails or runs out of time ends the run.  One JSON line per
measurement.
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


def workload(n):
    z = np.load(os.path.join(ROOT, "tests", "golden", "find_peaks.npz"))
    side = int(z["B/side"])
    g = int(np.ceil(np.sqrt(n)))
    rs = np.random.RandomState(17)
    sp = side / float(g)
    ij = np.stack(np.meshgrid(np.arange(g), np.arange(g), indexing="ij"), -1).reshape(-1, 2)[:n]
    q = np.empty((n, 3))
    q[:, 0] = float(z["B/f_seed"])
    q[:, 1:] = sp * (ij + 0.5 + 0.1 * rs.randn(n, 2))
    return z, q


def run_gpu(mode, n, repeats):
    import torch
    from rhmc_amd import capi
    z, q = workload(n)
    ctx = capi.Context(z["B/D"], device=0)
    ctx.set_option(capi.OPT_PEAKS_FUSED, 1 if mode == "fused" else 0)
    P = capi.make_params(dt=1., delta=1e-6, counter_max=1000, B_count=float(z["B/B_count"]),
                         f_lim=0., f_low=1., fwhm_pix=float(z["B/fwhm_pix"]), g_xx=1., g_ff=1.,
                         g_ff2=1., g0=1., g1=1., g2=1.)
    opts = capi.make_peaks_opts(float(z["B/f_lim"]), n_step=1000)
    dev = torch.device("cuda:0")
    stream = torch.cuda.Stream()
    q0 = torch.from_numpy(q).to(dev)
    s_d = torch.zeros(n, dtype=torch.int32, device=dev)
    t_d = torch.zeros(n, dtype=torch.int32, device=dev)
    times = []
    for r in range(repeats + 1):          # the first call warms up
        q_d = q0.clone()
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        with torch.cuda.stream(stream):
            e0.record(stream)
            ctx.find_peaks_device(P, opts, q_d.data_ptr(), n, s_d.data_ptr(), t_d.data_ptr(),
                                  None, stream.cuda_stream)
            e1.record(stream)
        stream.synchronize()
        if r:
            times.append(e0.elapsed_time(e1) * 1e-3)
    steps = s_d.cpu().numpy()
    status = t_d.cpu().numpy()
    ctx.close()
    t = float(np.median(times))
    return dict(mode=mode, seeds=n, total_steps=int(steps.sum()), seconds=t,
                steps_per_s=float(steps.sum() / t), times=times,
                faint=int((status & capi.PEAK_FAINT != 0).sum()),
                converged=int((status & capi.PEAK_CONVERGED != 0).sum()),
                cap=int((status & capi.PEAK_CAP != 0).sum()))


def run_cpu(n, cpu_seeds):
    import peaks_ref
    z, q = workload(n)
    ref = peaks_ref.PeaksRef(z["B/D"], float(z["B/B_count"]), float(z["B/fwhm_pix"]))
    t0 = time.perf_counter()
    _, steps, _, _ = ref.descend_all(q[:cpu_seeds], float(z["B/f_lim"]), n_step=1000)
    t = time.perf_counter() - t0
    return dict(mode="cpu_numpy", seeds=int(min(cpu_seeds, n)), of=n,
                total_steps=int(steps.sum()), seconds=t, steps_per_s=float(steps.sum() / t))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--one", nargs=2, metavar=("MODE", "N"), help="fused | stepwise | cpu, seeds")
    ap.add_argument("--sizes", type=int, nargs="+", default=[4096, 65536])
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--cpu-seeds", type=int, default=256)
    ap.add_argument("--limit", type=int, default=240, help="seconds per GPU measurement")
    a = ap.parse_args()
    if a.one:
        mode, n = a.one[0], int(a.one[1])
        r = run_cpu(n, a.cpu_seeds) if mode == "cpu" else run_gpu(mode, n, a.repeats)
        print(json.dumps(r), flush=True)
        return 0
    for n in a.sizes:
        for mode in ("fused", "stepwise"):
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--one", mode, str(n),
                                "--repeats", str(a.repeats)], timeout=a.limit)
            if r.returncode != 0:
                print("peaks_bench: %s at %d seeds ended with status %d; stopping"
                      % (mode, n, r.returncode), file=sys.stderr)
                return 1
    print(json.dumps(run_cpu(a.sizes[0], a.cpu_seeds)), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
