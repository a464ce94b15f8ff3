#!/usr/bin/env python3
"""Rates of the whole MH chain of HMC_random_batched and
RHMC_random_diag_batched: the host engine (the NumPy loop around one
trajectory launch and two energy calls per iteration) beside the device engine
(one rhmc_chain call) on the same NumPy draws, and the device engine with the
device's Philox draws.

4,096 chains on a 48-px image, K = 1, 3 and 10 stars, both metrics, 50
iterations of 10..49 steps.  The fields are Poisson images of magnitude
19.5-21.3 stars and every chain starts near the truth (tools/diag_bench.py's
fields); the unit metric gets the per-coordinate step vector that moves a star
at the truth as far per unit momentum as the diagonal metric does.  One timed
window is one whole run from the sampler's call to its return on the wall
clock: the draws, the uploads, the loop, the record's way back and its
transposition are all inside, as a user pays for them.  Each engine's windows
start from the same NumPy seed, so "host" and "device" run the same chains.

Every measurement is warmed up by a window first; the figure is the median of
--repeats windows and `times` holds them all.  Chain-steps per second is the
sum of the trajectory lengths actually run over the wall time, iterations per
second chains x iterations over it.  Each measurement runs in a child process
of its own under --limit seconds; the first one that fails or runs out of time
ends the run.  One JSON line per measurement, and after each shape's three one
line with the ratios device / host; the lines also go to
profiles/chain/chain_bench.jsonl.

  python tools/chain_bench.py
  python tools/chain_bench.py --one device unit 3
"""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "hmc-stellar-toy-model_amd"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

KS = (1, 3, 10)
SIDE, CHAINS, NITER, STEPS = 48, 4096, 50, (10, 50)
DT = 0.05
SEED = 7
OUT = os.path.join(ROOT, "profiles", "chain", "chain_bench.jsonl")


def run(engine, metric, K, repeats):
    from diag_bench import field
    from rhmc_amd import capi
    g, q0, _, dtv = field(K, SIDE, CHAINS)
    g.Nobjs, g.d, g.dt = K, 3 * K, dtv
    kw = dict(Niter=NITER, steps_min=STEPS[0], steps_max=STEPS[1])
    if metric == "diag":
        kw["dt_global"] = DT
        call = g.RHMC_random_diag_batched
    else:
        call = g.HMC_random_batched
    ctx, P = g._context(), g._params()
    opts = capi.make_chain_opts(metric, NITER, dt_global=DT, factor1=g.factor1,
                                steps_min=STEPS[0], steps_max=STEPS[1])
    times, total, accepted = [], 0, 0.
    for r in range(repeats + 1):          # the first window warms up
        np.random.seed(SEED)
        ctx.synchronize()
        t0 = time.perf_counter()
        if engine == "philox":            # the gym's call, plus the lengths for the rate
            out = ctx.chain(P, opts, q0, dt=None if metric == "diag" else dtv, seed=SEED,
                            record=("q_chain", "E_chain", "dE_chain", "accept", "steps"))
            q_chain = np.ascontiguousarray(np.transpose(out["q_chain"], (1, 0, 2)))
            A = np.ascontiguousarray(out["accept"].T).astype(float)
        else:
            call(q0, engine=engine, **kw)
            q_chain, A = g.q_chain, g.A_chain
        t1 = time.perf_counter()
        if r:
            times.append(t1 - t0)
        if engine == "philox":
            total = int(out["steps"].sum())
        else:                             # the lengths the run drew
            np.random.seed(SEED)
            np.random.randn(CHAINS, 3 * K)
            total = 0
            for _ in range(NITER):
                np.random.randn(CHAINS, 3 * K)
                total += int(np.random.randint(low=STEPS[0], high=STEPS[1], size=CHAINS).sum())
                np.random.random(CHAINS)
        accepted = float(np.mean(A))
        assert q_chain.shape == (CHAINS, NITER + 1, 3 * K)
    t = float(np.median(times))
    return dict(kind=engine, metric=metric, K=K, side=SIDE, chains=CHAINS, n_iter=NITER,
                steps=list(STEPS), seconds=t, chain_steps_per_s=total / t,
                iterations_per_s=CHAINS * NITER / t, accept=accepted, times=times)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--one", nargs=3, help="host|device|philox unit|diag K")
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--limit", type=int, default=150, help="seconds per measurement")
    a = ap.parse_args()
    if a.one:
        print(json.dumps(run(a.one[0], a.one[1], int(a.one[2]), a.repeats)), flush=True)
        return 0
    os.makedirs(os.path.dirname(OUT), exist_ok=True)
    with open(OUT, "w") as log:
        def emit(line):
            print(line, flush=True)
            log.write(line + "\n")
            log.flush()
        for metric in ("unit", "diag"):
            for K in KS:
                rate = {}
                for engine in ("host", "device", "philox"):
                    job = [engine, metric, str(K)]
                    try:
                        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--one"] +
                                           job + ["--repeats", str(a.repeats)], timeout=a.limit,
                                           capture_output=True, text=True)
                        rc, out = r.returncode, r.stdout
                        sys.stderr.write(r.stderr)
                    except subprocess.TimeoutExpired:
                        rc, out = 124, ""
                    if rc != 0:
                        print("chain_bench: %s ended with status %d; stopping"
                              % (" ".join(job), rc), file=sys.stderr)
                        return 1
                    line = out.strip().splitlines()[-1]
                    emit(line)
                    rate[engine] = json.loads(line)["chain_steps_per_s"]
                emit(json.dumps(dict(kind="ratio", metric=metric, K=K, side=SIDE, chains=CHAINS,
                                     device_over_host=rate["device"] / rate["host"],
                                     philox_over_host=rate["philox"] / rate["host"])))
    return 0


if __name__ == "__main__":
    sys.exit(main())
