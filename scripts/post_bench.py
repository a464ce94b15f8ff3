#!/usr/bin/env python3
"""Times librhmc_post's convergence call on the engine's record layout
[n_iter][n_chains][D] (fp64, device memory) and prints one JSON line per
measurement; --out appends them to a file (profiles/post/).

Per shape: the whole call (ms, passes made, bytes of kept samples x passes /
time), the first pass alone (max_lag = 16: moments and the first block of
lags; the yardstick is a device-to-device copy of the same bytes, timed here),
and the lag-block / workgroup variants.  At the first shape also the host
path: the device-to-host copy of the record plus diagnostics.convergence_stats
timed on a 256-chain subset and scaled by the chain count.

Needs a GPU; there is no fallback.  Warm-up calls come first, every figure is
the median of --repeats calls, each ended by a device synchronise."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "hmc-stellar-toy-model_amd")]

SHAPES = [(4096, 1000, 3), (131072, 100, 3), (16384, 200, 30)]   # n_chains, n_iter, D


def chains(torch, n_chains, n_iter, D, ar=0.5, seed=1):
    """AR(1) chains around (1000, 24, 24, ...) in the record layout."""
    g = torch.Generator(device="cuda").manual_seed(seed)
    x = torch.empty((n_iter, n_chains, D), dtype=torch.float64, device="cuda")
    x[0] = torch.randn((n_chains, D), dtype=torch.float64, device="cuda", generator=g)
    for t in range(1, n_iter):
        e = torch.randn((n_chains, D), dtype=torch.float64, device="cuda", generator=g)
        x[t] = ar * x[t - 1] + (1 - ar * ar) ** 0.5 * e
    centre = torch.tensor([1000., 24., 24.] * (D // 3 + 1), dtype=torch.float64,
                          device="cuda")[:D]
    return x + centre


def median_ms(fn, sync, warmup, repeats):
    for _ in range(warmup):
        fn()
    sync()
    ts = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        fn()
        sync()
        ts.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(ts)), float(np.min(ts)), float(np.max(ts))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--thin", type=int, default=1)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=10)
    ap.add_argument("--shapes", type=int, nargs="*", default=[0, 1, 2])
    ap.add_argument("--no-host", action="store_true", help="skip the host-path timing")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    from rhmc_amd import capi, diagnostics, post
    if not capi.device_available():
        sys.exit("post_bench: no GPU visible")
    lines = []

    def emit(**kw):
        line = json.dumps(kw)
        print(line, flush=True)
        lines.append(line)

    sync = torch.cuda.synchronize
    for si in a.shapes:
        n_chains, n_iter, D = SHAPES[si]
        x = chains(torch, n_chains, n_iter, D)
        kept = len(range(0, n_iter, a.thin)) // 2 * 2
        kept_bytes = kept * n_chains * D * 8
        shape = dict(n_chains=n_chains, n_iter=n_iter, D=D, thin=a.thin, kept_bytes=kept_bytes)
        # the yardstick: a device-to-device copy of the kept bytes (read + write)
        src = x[:kept * a.thin:a.thin].contiguous()
        dst = torch.empty_like(src)
        ms, lo, hi = median_ms(lambda: dst.copy_(src), sync, a.warmup, a.repeats)
        emit(what="d2d_copy", ms=ms, ms_min=lo, ms_max=hi, read_GBps=kept_bytes / ms / 1e6,
             **shape)
        del src, dst
        for t_blk in (16, 8):
            for block in (256, 128, 64):
                ctx = post.PostContext(0, t_blk=t_blk, block=block)
                run = lambda ml: diagnostics.convergence_stats_device(   # noqa: E731
                    x, thin_rate=a.thin, warm_up_num=0, layout="iter", max_lag=ml, detail=True,
                    ctx=ctx)
                det = run(0)[2]
                ms, lo, hi = median_ms(lambda: run(0), sync, a.warmup, a.repeats)
                emit(what="convergence", t_blk=t_blk, block=block, ms=ms, ms_min=lo, ms_max=hi,
                     passes=det["passes"], lags_max=int(det["lags_used"].max()),
                     GBps=kept_bytes * det["passes"] / ms / 1e6, **shape)
                ms, lo, hi = median_ms(lambda: run(t_blk), sync, a.warmup, a.repeats)
                emit(what="first_pass", t_blk=t_blk, block=block, ms=ms, ms_min=lo, ms_max=hi,
                     passes=1, GBps=kept_bytes / ms / 1e6, **shape)
                ctx.close()
        if si == 0 and not a.no_host:
            # the host path: copy the record down, then the NumPy loops
            ms_copy, lo, hi = median_ms(lambda: x.cpu(), sync, 1, 3)
            sub = 256
            h = np.ascontiguousarray(x[:, :sub].cpu().numpy().transpose(1, 0, 2))
            t0 = time.perf_counter()
            R, neff = diagnostics.convergence_stats(h, thin_rate=a.thin, warm_up_num=0)
            ms_np = (time.perf_counter() - t0) * 1e3
            got = diagnostics.convergence_stats_device(x[:, :sub].contiguous(),
                                                       thin_rate=a.thin, layout="iter")
            emit(what="host_path", d2h_copy_ms=ms_copy, numpy_ms_256_chains=ms_np,
                 numpy_ms_scaled=ms_np * n_chains / sub,
                 total_ms=ms_copy + ms_np * n_chains / sub,
                 R_rel_err=float(np.max(np.abs(got[0] / R - 1))),
                 neff_rel_err=float(np.max(np.abs(got[1] / neff - 1))), **shape)
        del x
        torch.cuda.empty_cache()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
