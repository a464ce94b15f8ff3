#!/usr/bin/env python3
"""Run one launch through the library named by RHMC_LIB and save its outputs
(tools only; compare two builds bit for bit with tools/lib_cmp.py).

--op leapfrog (default): a workload's full leapfrog launch; q, p, iteration
counts and status.
  RHMC_LIB=build/variants/lib_x.so python tools/lib_dump.py C2 out.npz [--chains N]
--op hmc_random / diag_random: the trajectories of a KxSIDE field built as
tools/diag_bench.py builds it, with unequal lengths of at most 40 steps; q, p,
status and, for diag_random with --trace, the trace.  --wall puts a flux wall
just under every chain's faintest star and sends that star towards it.
  python tools/lib_dump.py 3x48 out.npz --op diag_random --kernel multiwin --chains 5"""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..",
                                "hmc-stellar-toy-model_amd"))
import torch  # noqa: E402
from rhmc_amd import capi, workloads  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("workload", help="a workload name (leapfrog) or KxSIDE (trajectories)")
ap.add_argument("out")
ap.add_argument("--op", choices=["leapfrog", "hmc_random", "diag_random"], default="leapfrog")
ap.add_argument("--kernel", default="auto", help="kernel family (capi.KERNELS)")
ap.add_argument("--chains", type=int, default=None)
ap.add_argument("--dt", type=float, default=None, help="trajectories: the step (diag_bench's)")
ap.add_argument("--trace", action="store_true", help="diag_random: save the trace too")
ap.add_argument("--wall", action="store_true", help="trajectories: a flux wall that chains cross")


def leapfrog(args):
    wl = workloads.make(args.workload, n_chains=args.chains)
    P = capi.make_params(**wl.params)
    dev = torch.device("cuda:0")
    ctx = capi.Context(wl.D, device=0)
    ctx.set_kernel(args.kernel)
    q = torch.from_numpy(wl.q0).to(dev)
    p = torch.from_numpy(wl.p0).to(dev)
    it = torch.zeros((wl.n_chains, 2), dtype=torch.int32, device=dev)
    st = torch.zeros(wl.n_chains, dtype=torch.int32, device=dev)
    ctx.leapfrog_device(P, q.data_ptr(), p.data_ptr(), wl.n_chains, wl.K, wl.n_steps,
                        it.data_ptr(), st.data_ptr(), stream=0)
    torch.cuda.synchronize()
    np.savez(args.out, q=q.cpu().numpy(), p=p.cpu().numpy(), it=it.cpu().numpy(),
             st=st.cpu().numpy())
    print("%s: %d chains x %d steps -> %s" % (args.workload, wl.n_chains, wl.n_steps, args.out))


def trajectories(args):
    import diag_bench
    from rhmc_amd.photometry import mag2flux
    K, side = (int(v) for v in args.workload.split("x"))
    n = args.chains or 5
    dt = args.dt or diag_bench.DT
    g, q0, p0, dtv = diag_bench.field(K, side, n)
    dtv = dtv * (dt / diag_bench.DT)
    if args.wall:   # the faintest star starts just above the wall, moving down
        g.f_lim = mag2flux(21.7) * g.flux_to_count
        faint = 3 * int(np.argmin(q0[0, 0::3]))
        q0[:, faint] = g.f_lim * (1.002 + 0.002 * np.arange(n))
        p0[:, faint] = (-2.0 - 0.1 * np.arange(n)) * np.sqrt(g._mass_batch(q0)[:, faint])
    steps = (1 + (11 * np.arange(n) + 5) % 40).astype(np.int32)
    ctx, P = g._context(), g._params()
    ctx.set_kernel(args.kernel)
    out = {}
    if args.op == "hmc_random":
        out["q"], out["p"], out["st"] = ctx.hmc_random(P, dtv, q0, p0, steps, return_status=True)
    else:
        r = ctx.diag_random(P, dt, g.factor1, q0, p0, steps, return_status=True,
                            trace=args.trace)
        out["q"], out["p"], out["st"] = r[:3]
        if args.trace:
            out["trace"] = r[3]
    np.savez(args.out, **out)
    below = ""
    if "trace" in out:      # NaN rows (past a chain's length) compare false
        below = ", %d below the wall" % int((out["trace"][:, 1:, 0::3] < g.f_lim).any(axis=(1, 2)).sum())
    print("%s %s %s: %d chains, steps %s, %d reflected%s, %d non-finite -> %s" % (
        args.op, args.workload, args.kernel, n, steps.tolist(),
        int((out["st"] & capi.STATUS_REFLECT_F != 0).sum()), below,
        int((out["st"] & capi.STATUS_NONFINITE != 0).sum()), args.out))


def main(argv=None):
    args = ap.parse_args(argv)
    (leapfrog if args.op == "leapfrog" else trajectories)(args)


if __name__ == "__main__":
    main()
