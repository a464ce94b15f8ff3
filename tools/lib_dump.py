#!/usr/bin/env python3
"""Run one launch through the library named by RHMC_LIB and save its outputs
(tools only; compare two builds bit for bit with tools/lib_cmp.py).

--op leapfrog (default): a workload's full leapfrog launch; q, p, iteration
counts and status.  KxSIDE names the workload S<SIDE>K<K> (5 chains unless
--chains says otherwise), on which --no-prior, --vc (the pair potential),
--fwhm, --steps and --inexact (an image that fp32 does not hold) apply.
  RHMC_LIB=build/variants/lib_x.so python tools/lib_dump.py C2 out.npz [--chains N]
  python tools/lib_dump.py 3x40 out.npz --kernel generic --vc
--op energy: V and T of the same starts (--no-T: V alone), --f-pos the bits of
rhmc_energy (1: flux wall, 2: no position check).  --op gradient: dVdq and
dphidq (grad0, grad1).  Both follow --kernel like the step: `auto` sends one
star on an fp32-exact 32/48/64-px image to the register-window energy, so a
comparison of the LDS-image bodies (ldsimage/MAXK) passes --kernel generic.
--op hmc_random / diag_random: the trajectories of a KxSIDE field built as
tools/diag_bench.py builds it, with unequal lengths of at most 40 steps; q, p,
status and, for diag_random with --trace, the trace.  --wall puts a flux wall
just under the star that is faintest in chain 0, in every chain, and sends that
star towards it.
  python tools/lib_dump.py 3x48 out.npz --op diag_random --kernel multiwin --chains 5
--op integrate: --steps (default 10) steps of the explicit integrator --solver
(hmc, naive or leap_frog) at the step --dt on the KxSIDE field of the leapfrog
op, unit-normal momenta for hmc; q, p and status.  --wall turns f_pos on, puts
the wall at half the faintest flux of the field and, in every chain, starts the
star that is faintest in chain 0 just above it, moving down (hmc crosses the
wall too, which it never tests: its status must stay 0).
  python tools/lib_dump.py 70x32 out.npz --op integrate --solver naive --wall --steps 9"""
import argparse
import os
import re
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..",
                                "hmc-stellar-toy-model_amd"))
import torch  # noqa: E402
from rhmc_amd import capi, workloads  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("workload", help="a workload name (leapfrog) or KxSIDE (trajectories)")
ap.add_argument("out")
ap.add_argument("--op", default="leapfrog",
                choices=["leapfrog", "energy", "gradient", "hmc_random", "diag_random",
                         "integrate"])
ap.add_argument("--solver", default="leap_frog", choices=["hmc", "naive", "leap_frog"],
                help="integrate: the explicit integrator")
ap.add_argument("--kernel", default="auto", help="kernel family (capi.KERNELS)")
ap.add_argument("--chains", type=int, default=None)
ap.add_argument("--dt", type=float, default=None, help="trajectories: the step (diag_bench's); integrate: dt")
ap.add_argument("--trace", action="store_true", help="diag_random: save the trace too")
ap.add_argument("--wall", action="store_true", help="trajectories, integrate: a flux wall that chains cross")
ap.add_argument("--no-prior", action="store_true", help="KxSIDE: the flux prior off")
ap.add_argument("--vc", action="store_true", help="KxSIDE: the pair potential on")
ap.add_argument("--fwhm", type=float, default=None, help="KxSIDE: the PSF's FWHM in px")
ap.add_argument("--steps", type=int, default=None, help="leapfrog, integrate: steps of the launch")
ap.add_argument("--inexact", action="store_true", help="KxSIDE: D + 0.1, not exact in fp32")
ap.add_argument("--f-pos", type=int, default=0, help="energy: rhmc_energy's f_pos bits")
ap.add_argument("--no-T", action="store_true", help="energy: V alone (no momenta)")


def workload(args):
    """The named workload, or S<SIDE>K<K> for KxSIDE with the options applied."""
    m = re.fullmatch(r"(\d+)x(\d+)", args.workload)
    if not m:
        return workloads.make(args.workload, n_chains=args.chains)
    K, side = int(m.group(1)), int(m.group(2))
    wl = workloads.make("S%dK%d" % (side, K), n_chains=args.chains or 5)
    wl.params.update(use_prior=not args.no_prior, use_Vc=args.vc)
    if args.fwhm:
        wl.params["fwhm_pix"] = args.fwhm
    if args.inexact:
        wl.D = wl.D + 0.1
    return wl


def leapfrog(args):
    wl = workload(args)
    if args.steps is not None:
        wl.n_steps = args.steps
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


def energy(args):
    wl = workload(args)
    ctx = capi.Context(wl.D, device=0, kernel=args.kernel)
    dev = torch.device("cuda:0")
    q, p = torch.from_numpy(wl.q0).to(dev), torch.from_numpy(wl.p0).to(dev)
    V = torch.zeros(wl.n_chains, dtype=torch.float64, device=dev)
    T = torch.zeros_like(V)
    ctx.energy_device(capi.make_params(**wl.params), q.data_ptr(),
                      0 if args.no_T else p.data_ptr(), V.data_ptr(),
                      0 if args.no_T else T.data_ptr(), wl.n_chains, wl.K, f_pos=args.f_pos)
    torch.cuda.synchronize()
    np.savez(args.out, V=V.cpu().numpy(), T=T.cpu().numpy())
    print("energy %s %s f_pos %d: %d chains, %d infinite -> %s" % (
        args.workload, args.kernel, args.f_pos, wl.n_chains, int(torch.isinf(V).sum()), args.out))


def gradient(args):
    wl = workload(args)
    ctx = capi.Context(wl.D, device=0, kernel=args.kernel)
    P = capi.make_params(**wl.params)
    np.savez(args.out, grad0=ctx.gradient(P, wl.q0, 0), grad1=ctx.gradient(P, wl.q0, 1))
    print("gradient %s %s: %d chains -> %s" % (args.workload, args.kernel, wl.n_chains, args.out))


def integrate(args):
    wl = workload(args)
    par, n, n_steps = wl.params, wl.n_chains, 10 if args.steps is None else args.steps
    if args.dt:
        par["dt"] = args.dt
    hmc = args.solver == "hmc"
    q0 = wl.q0.copy()
    p0 = wl.p0 / np.sqrt(workloads.metric_diag(q0, par)) if hmc else wl.p0.copy()
    if args.wall:   # the faintest star starts just above the wall, moving down
        par["f_lim"] = 0.5 * q0[:, 0::3].min()
        faint = 3 * int(np.argmin(q0[0, 0::3]))
        q0[:, faint] = par["f_lim"] * (1.002 + 0.002 * np.arange(n))
        if hmc:     # unit metric: the momentum that carries it as far below, were it free
            p0[:, faint] = -2. * (q0[:, faint] - par["f_lim"]) / (par["dt"] * max(n_steps, 1))
        else:
            p0[:, faint] = (-2.0 - 0.1 * np.arange(n)) * np.sqrt(
                workloads.metric_diag(q0, par)[:, faint])
    ctx = capi.Context(wl.D, device=0, kernel=args.kernel)
    solver = {"hmc": capi.SOLVER_HMC, "naive": capi.SOLVER_RHMC_NAIVE,
              "leap_frog": capi.SOLVER_RHMC_LEAPFROG}[args.solver]
    q, p, st = ctx.integrate(capi.make_params(**par), solver, q0, p0, n_steps, f_pos=args.wall,
                             return_status=True)
    np.savez(args.out, q=q, p=p, st=st)
    print("integrate %s %s %s: %d chains x %d steps, %d chains with REFLECT_F, %d non-finite -> %s"
          % (args.solver, args.workload, args.kernel, n, n_steps,
             int((st & capi.STATUS_REFLECT_F != 0).sum()),
             int((st & capi.STATUS_NONFINITE != 0).sum()), args.out))


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
    {"leapfrog": leapfrog, "energy": energy, "gradient": gradient,
     "integrate": integrate}.get(args.op, trajectories)(args)


if __name__ == "__main__":
    main()
