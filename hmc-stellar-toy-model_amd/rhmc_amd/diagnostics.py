"""MCMC post-processing of gathered chains: Gelman-Rubin
R-hat, effective sample size and acceptance rates, as the reference computes
them (utils.py:86-209).  Host-side NumPy on the gathered samples — not part of
the per-step hot path.  convergence_stats_device / acceptance_rate_device
compute the same on the GPU from chains that are already in device memory
(librhmc_post.so, include/rhmc_post.h), for chain counts where the NumPy loops
and the copy to the host no longer keep up."""
import numpy as np


def variogram(chains, var_num, t_lag):
    """utils.py:170-188 (BDA eq. 11.7)."""
    m = len(chains)
    n = chains[0].shape[0]
    V_t = 0.
    for i in range(m):
        c = chains[i][:, var_num]
        V_t += np.sum(np.square(c[t_lag:] - c[:-t_lag]))
    return V_t / float(m * (n - t_lag))


def convergence_stats(q_chain, thin_rate=5, warm_up_num=0):
    """utils.py:86-168: (R_hat[D], n_eff[D]) of q_chain [Nchain, Niter, D];
    each chain is warmed up, thinned, trimmed to even length and split in two.
    `n = L_chain/2` is Python 2 integer division in the reference."""
    Nchain, Niter, D = q_chain.shape
    assert Nchain > 1
    chains = []
    for mm in range(Nchain):
        c = q_chain[mm, warm_up_num:, :][::thin_rate, :]
        L = c.shape[0]
        if L % 2:
            c = c[:L - 1]
        n = L // 2
        chains.append(c[:n])
        chains.append(c[n:])
    m = len(chains)
    W = np.mean(np.array([np.std(c, ddof=1, axis=0) for c in chains]), axis=0)
    mean_within = np.array([np.mean(c, axis=0) for c in chains])
    mean_all = np.mean(mean_within, axis=0)
    B = np.sum(np.square(mean_within - mean_all), axis=0) * n / float(m - 1)
    var = W * (n - 1) / float(n) + B / float(n)
    R = np.sqrt(var / W)
    n_eff = np.zeros(D, dtype=float)
    for i in range(D):
        rho_t1 = 1. - variogram(chains, i, 1) / (2 * var[i])
        rho_t2 = 1. - variogram(chains, i, 2) / (2 * var[i])
        if rho_t1 < 5e-2:
            sum_rho = 0
        else:
            rho_t = [rho_t1, rho_t2]
            t = 1
            while t < n - 2:
                rho_t.append(1 - variogram(chains, i, t + 2) / (2 * var[i]))
                if ((t % 2) == 1) & ((rho_t[t] + rho_t[t + 1]) < 0):
                    break
                t += 1
            sum_rho = np.sum(rho_t[:t])
            if sum_rho < 0:
                sum_rho = 0
        n_eff[i] = m * n / (1 + 2 * sum_rho)
    return R, n_eff


def acceptance_rate(decision_chain, start=None, end=None):
    """utils.py:192-209: decision_chain [Nchain, Niter, 1] of 0/1."""
    _, Niter, _ = decision_chain.shape
    if start is None and end is None:
        return np.sum(decision_chain, axis=(1, 2)) / Niter
    Niter = end - start if end > 0 else Niter - start
    return np.sum(decision_chain[:, start:end, :], axis=(1, 2)) / Niter


def _post():
    # loaded on first use: the package imports without librhmc_post.so
    from . import post
    return post


def _device_view(a):
    """(ptr, shape, strides in elements, device index) of a device array:
    anything with data_ptr() and shape (a torch tensor), or a tuple
    (ptr, shape[, strides in elements])."""
    if isinstance(a, tuple):
        ptr, shape = int(a[0]), tuple(int(v) for v in a[1])
        strides = tuple(int(v) for v in a[2]) if len(a) > 2 and a[2] is not None else None
        dev = None
    else:
        ptr, shape = int(a.data_ptr()), tuple(int(v) for v in a.shape)
        strides = tuple(int(v) for v in a.stride()) if hasattr(a, "stride") else None
        dev = getattr(getattr(a, "device", None), "index", None)
    if strides is None:
        strides = tuple(int(np.prod(shape[i + 1:])) for i in range(len(shape)))
    return ptr, shape, strides, dev


def convergence_stats_device(q_chain, thin_rate=5, warm_up_num=0, layout="chain", max_lag=0,
                             detail=False, ctx=None, stream=None):
    """convergence_stats on the GPU (librhmc_post.so) -> NumPy (R[D], n_eff[D]),
    with detail a third item (post.PostContext.convergence_device).

    q_chain: fp64, [Nchain, Niter, D] with layout="chain" (the reference's) or
    [n_iter, n_chains, D] with layout="iter" (the engine's MhRecord.q_chain).
    A NumPy array goes through the host entry (uploaded, run, freed); anything
    with data_ptr() and shape (a torch tensor on the GPU), or a tuple
    (ptr, shape[, strides in elements]), is read where it is: no copy of the
    chains to the host is made.  The last axis must have stride 1; the other
    two any non-negative strides (padded rows: a view [:, :, :D] of wider
    rows).  max_lag > 0 caps the lag search (0: the reference's unbounded
    one).  ctx: a post.PostContext (default: one per device, kept); stream: a
    hipStream_t handle (default: the null stream); the call synchronises it."""
    if layout not in ("chain", "iter"):
        raise ValueError('layout must be "chain" or "iter"')
    P = _post()
    host = isinstance(q_chain, np.ndarray)
    if host:
        if q_chain.dtype != np.float64:
            raise TypeError("q_chain must be float64, got %s" % q_chain.dtype)
        x = q_chain
        if x.ndim != 3:
            raise ValueError("q_chain must have 3 axes")
        if (x.shape[2] > 1 and x.strides[2] != 8) or any(s < 0 or s % 8 for s in x.strides[:2]):
            x = np.ascontiguousarray(x)
        ptr, shape, dev = x, x.shape, None
        strides = tuple(s // 8 for s in x.strides)
    else:
        if getattr(q_chain, "dtype", None) is not None and "float64" not in str(q_chain.dtype):
            raise TypeError("q_chain must be float64, got %s" % q_chain.dtype)
        ptr, shape, strides, dev = _device_view(q_chain)
        if len(shape) != 3:
            raise ValueError("q_chain must have 3 axes")
        if shape[2] > 1 and strides[2] != 1:
            raise ValueError("the coordinate axis must have stride 1")
    ax_c, ax_i = (0, 1) if layout == "chain" else (1, 0)
    lay = P.PostLayout(shape[ax_i], shape[ax_c], shape[2], strides[ax_i], strides[ax_c])
    if ctx is None:
        ctx = P.default_context(dev or 0)
    if host:
        # the host entry uploads the layout's extent from the first element
        return ctx.convergence(x, lay, warm_up_num, thin_rate, max_lag, detail)
    return ctx.convergence_device(ptr, lay, warm_up_num, thin_rate, max_lag, detail, stream)


def acceptance_rate_device(accept, start=None, end=None, ctx=None, stream=None):
    """Acceptance rate per chain of the engine's record accept [n_iter, n_chains]
    (int32: MhRecord.accept) on the GPU -> NumPy [n_chains].  start / end: None
    (the whole run) or 0 <= start < end <= n_iter, both given.  A NumPy array
    is uploaded; a device array (data_ptr() and shape, or (ptr, shape[,
    strides])) is read where it is.  The reference's decision_chain
    [Nchain, Niter, 1] is accept = decision_chain[:, :, 0].T."""
    if (start is None) != (end is None):
        raise ValueError("give both start and end, or neither")
    s, e = (-1, -1) if start is None else (int(start), int(end))
    if start is not None and not 0 <= s < e:
        raise ValueError("0 <= start < end <= n_iter")
    P = _post()
    if isinstance(accept, np.ndarray):
        if ctx is None:
            ctx = P.default_context(0)
        return ctx.acceptance(accept, s, e)
    if getattr(accept, "dtype", None) is not None and "int32" not in str(accept.dtype):
        raise TypeError("accept must be int32, got %s" % accept.dtype)
    ptr, shape, strides, dev = _device_view(accept)
    if len(shape) != 2 or (shape[1] > 1 and strides[1] != 1):
        raise ValueError("accept must be [n_iter][n_chains] with chain stride 1")
    if ctx is None:
        ctx = P.default_context(dev or 0)
    return ctx.acceptance_fetch(ptr, shape[0], shape[1], strides[0], s, e, stream)
