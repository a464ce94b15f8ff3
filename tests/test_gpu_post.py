"""librhmc_post.so on the GPU (include/rhmc_post.h, rhmc_amd/post.py and the
*_device functions of rhmc_amd/diagnostics.py) against the reference's outputs
(tests/golden/solvers.npz) and the NumPy restatement
diagnostics.convergence_stats, with torch tensors as device buffers.

Tolerances (every case): R rtol 1e-11, n_eff rtol 1e-9, the number of lags the
search read equal to the NumPy loop's.  Why they hold: a moment or a variogram
here sums at most 1,500 terms, so reordering moves it by <= ~2e-13 relative;
the sum of the rho_t has at most 155 terms, so n_eff moves by <= ~6e-11; and
every case first asserts, on the NumPy side, that the rule's deciding
quantities (rho_1 - 0.05, and rho_{t+1} + rho_{t+2} at every odd t tested) are
at least 1e-6 from their thresholds, nine orders above the arithmetic noise,
so the lag count cannot flip."""
import functools

import numpy as np
import pytest
import torch

from conftest import load_golden

pytestmark = pytest.mark.gpu

R_RTOL = 1e-11
NEFF_RTOL = 1e-9
MARGIN = 1e-6


# ------------------------------------------------------------------ NumPy side
def split_sequences(x, thin, warm):
    """convergence_stats's split sequences [m][n][D] of x [Nchain][Niter][D]."""
    c = x[:, warm:][:, ::thin]
    L = c.shape[1] - c.shape[1] % 2
    n = L // 2
    return c[:, :L].reshape(x.shape[0] * 2, n, x.shape[2])


def rule_trace(x, thin, warm):
    """The reference's lag search per coordinate -> (lags read [D], margin):
    lags = the variograms its loop evaluates (2 when rho_1 < 0.05), margin =
    the smallest distance of a deciding quantity from its threshold."""
    y = split_sequences(x, thin, warm)
    m, n, D = y.shape
    W = np.mean(np.std(y, ddof=1, axis=1), axis=0)
    mw = np.mean(y, axis=1)
    B = np.sum(np.square(mw - np.mean(mw, axis=0)), axis=0) * n / float(m - 1)
    var = W * (n - 1) / float(n) + B / float(n)
    lags = np.zeros(D, np.int64)
    margin = np.inf
    for d in range(D):
        if not (np.isfinite(var[d]) and var[d] > 0):
            continue

        @functools.lru_cache(maxsize=None)
        def rho(t, d=d):
            v = np.sum(np.square(y[:, t:, d] - y[:, :-t, d])) / float(m * (n - t))
            return 1. - v / (2 * var[d])
        margin = min(margin, abs(rho(1) - 5e-2))
        lags[d] = 2
        if rho(1) < 5e-2:
            continue
        t = 1
        while t < n - 2:
            lags[d] = t + 2
            if t % 2 == 1:
                margin = min(margin, abs(rho(t + 1) + rho(t + 2)))
                if rho(t + 1) + rho(t + 2) < 0:
                    break
            t += 1
    return lags, margin


def ar1(seed, n_chains, n_iter, D, ar, offset=0.):
    """AR(1) chains [n_chains][n_iter][D] by tests/golden/make_goldens.py's
    recipe (unit marginal variance, small between-chain offsets)."""
    rs = np.random.RandomState(seed)
    shape = (n_chains, n_iter, D)
    e = rs.randn(*shape)
    x = np.empty(shape)
    x[:, 0] = e[:, 0]
    for t in range(1, n_iter):
        x[:, t] = ar * x[:, t - 1] + np.sqrt(1 - ar * ar) * e[:, t]
    x += rs.randn(n_chains, 1, D) * 0.1
    return x + offset


# (n_chains, n_iter, D, thin, warm, ar, seed, offset)
SHAPES = {
    "min_n3": (2, 7, 1, 1, 0, 0.5, 5, 0.),            # n = 3, the minimum
    "odd_trim": (3, 10, 2, 1, 1, 0.5, 5, 0.),         # 9 kept rows, trimmed to 8
    "c67": (67, 61, 3, 3, 5, 0.7, 5, 0.),
    "k10": (257, 40, 30, 2, 3, 0.3, 5, 0.),           # K = 10, D = 30
    "offset": (1031, 96, 6, 1, 0, 0.3, 5, 1000.),     # cancellation, > 1 workgroup
}


@functools.lru_cache(maxsize=None)
def shape_case(name):
    """(x [n_chains][n_iter][D], thin, warm, R, n_eff, lags, margin), computed once."""
    from rhmc_amd import diagnostics as Dg
    n_chains, n_iter, D, thin, warm, ar, seed, offset = SHAPES[name]
    x = ar1(seed, n_chains, n_iter, D, ar, offset)
    R, neff = Dg.convergence_stats(x, thin_rate=thin, warm_up_num=warm)
    lags, margin = rule_trace(x, thin, warm)
    x.setflags(write=False)
    return x, thin, warm, R, neff, lags, margin


def to_iter(x):
    """[n_chains][n_iter][D] -> the engine's record [n_iter][n_chains][D] on the GPU."""
    return torch.from_numpy(np.ascontiguousarray(x.transpose(1, 0, 2))).cuda()


def check(got, R, neff, lags=None):
    print("R rel err %.3e  n_eff rel err %.3e" % (
        np.nanmax(np.abs(got[0] / R - 1)), np.nanmax(np.abs(got[1] / neff - 1))))
    np.testing.assert_allclose(got[0], R, rtol=R_RTOL)
    np.testing.assert_allclose(got[1], neff, rtol=NEFF_RTOL)
    if lags is not None:
        print("lags", got[2]["lags_used"], "passes", got[2]["passes"])
        assert np.array_equal(got[2]["lags_used"], lags)


@pytest.fixture(scope="module")
def Dg(gpu_lib):
    from rhmc_amd import diagnostics
    return diagnostics


# ------------------------------------------------------------------- the cases
@pytest.mark.parametrize("thin,warm,kR,kN", [(2, 10, "R", "neff"), (1, 0, "R1", "neff1")])
@pytest.mark.parametrize("name", ["iid", "ar", "ar_hi"])
def test_reference_goldens(Dg, name, thin, warm, kR, kN):
    z = load_golden("solvers")
    x = z["conv_" + name + "/x"]
    R, neff = z["conv_%s/%s" % (name, kR)], z["conv_%s/%s" % (name, kN)]
    lags, margin = rule_trace(x, thin, warm)
    print("margin %.3e lags %s" % (margin, lags))
    assert margin >= MARGIN
    host = Dg.convergence_stats_device(x, thin_rate=thin, warm_up_num=warm, detail=True)
    check(host, R, neff, lags)
    dev = Dg.convergence_stats_device(torch.from_numpy(x).cuda(), thin_rate=thin,
                                      warm_up_num=warm, detail=True)
    check(dev, R, neff, lags)
    # the same chains in the engine's layout
    it = Dg.convergence_stats_device(to_iter(x), thin_rate=thin, warm_up_num=warm,
                                     layout="iter", detail=True)
    check(it, R, neff, lags)
    n = (len(range(warm, x.shape[1], thin)) // 2)
    assert host[2]["n"] == dev[2]["n"] == n
    # one pass for the moments and the first 16 lags, one more per 16 lags after
    assert dev[2]["passes"] == max(1, -(-int(lags.max()) // 16))


def test_goldens_cross_block_boundaries_and_reach_exhaustion():
    """The lag counts of the six golden runs span several 16-lag blocks."""
    z = load_golden("solvers")
    seen = set()
    for name in ("iid", "ar", "ar_hi"):
        for thin, warm in ((2, 10), (1, 0)):
            seen |= set(rule_trace(z["conv_" + name + "/x"], thin, warm)[0].tolist())
    assert min(seen) == 2 and max(seen) > 32 and len([s for s in seen if s > 16]) >= 3, seen


@pytest.mark.parametrize("name", ["iid", "ar", "ar_hi"])
def test_variogram_device(gpu_lib, name):
    """Golden vg: utils.variogram of the two unsplit chains x[0, :100] and
    x[1, :100], coordinate 1, lags 1, 2, 5.  The split sequences of two copies
    of the chain [x[0, :100]; x[1, :100]] are those two chains, twice."""
    from rhmc_amd import post
    z = load_golden("solvers")
    x = z["conv_" + name + "/x"]
    chain = np.concatenate([x[0, :100], x[1, :100]])             # [200][D]
    d_x = torch.from_numpy(np.stack([chain, chain])).cuda()       # [2][200][D]
    D = x.shape[2]
    lay = post.PostLayout(200, 2, D, D, 200 * D)
    ctx = post.PostContext(0)
    V = ctx.variogram_device(d_x.data_ptr(), lay, 1, 5)
    np.testing.assert_allclose(V[[0, 1, 4], 1], z["conv_" + name + "/vg"], rtol=1e-12)
    # any first lag, across a block boundary, up to the last lag n - 1 = 99
    V2 = ctx.variogram_device(d_x.data_ptr(), lay, 5, 95)
    assert np.array_equal(V2[0], V[4])
    y = np.stack([x[0, :100], x[1, :100]])
    for t in (17, 32, 33, 98, 99):
        ref = np.sum(np.square(y[:, t:] - y[:, :-t]), axis=(0, 1)) / (2. * (100 - t))
        np.testing.assert_allclose(V2[t - 5], ref, rtol=1e-12)
    ctx.close()


@pytest.mark.parametrize("name", list(SHAPES))
def test_shapes_iter_layout(Dg, name):
    x, thin, warm, R, neff, lags, margin = shape_case(name)
    print("margin %.3e" % margin)
    assert margin >= MARGIN
    got = Dg.convergence_stats_device(to_iter(x), thin_rate=thin, warm_up_num=warm,
                                      layout="iter", detail=True)
    check(got, R, neff, lags)
    y = split_sequences(x, thin, warm)
    # a mean of n <= 48 samples carries an absolute error of about n eps max|y|
    # (< 1e-14 max|y|), whatever its own size: some split means are near zero
    np.testing.assert_allclose(got[2]["split_mean"], y.mean(axis=1), rtol=1e-12,
                               atol=1e-14 * np.abs(y).max())
    np.testing.assert_allclose(got[2]["split_sd"], y.std(axis=1, ddof=1), rtol=1e-11)


def test_padded_rows(Dg):
    x, thin, warm, R, neff, lags, _ = shape_case("c67")
    n_chains, n_iter, D = x.shape
    plain = Dg.convergence_stats_device(to_iter(x), thin, warm, layout="iter", detail=True)
    wide = torch.full((n_iter, n_chains, D + 5), float("nan"), dtype=torch.float64,
                      device="cuda")
    wide[:, :, :D] = to_iter(x)
    view = wide[:, :, :D]
    assert view.stride() == (n_chains * (D + 5), D + 5, 1)
    got = Dg.convergence_stats_device(view, thin, warm, layout="iter", detail=True)
    check(got, R, neff, lags)
    # the same columns in the same workgroup positions: the same bits
    assert np.array_equal(got[0], plain[0]) and np.array_equal(got[1], plain[1])
    # a raw (pointer, shape, strides) triple
    raw = Dg.convergence_stats_device((wide.data_ptr(), (n_iter, n_chains, D),
                                       (n_chains * (D + 5), D + 5, 1)), thin, warm,
                                      layout="iter")
    assert np.array_equal(raw[0], plain[0]) and np.array_equal(raw[1], plain[1])


def test_zero_columns(Dg):
    """D = 6 whose last three columns are zero (reversible-jump padding)."""
    x, thin, warm, R, neff, lags, _ = shape_case("c67")
    n_chains, n_iter, D = x.shape
    three = Dg.convergence_stats_device(to_iter(x), thin, warm, layout="iter", detail=True)
    x6 = np.concatenate([x, np.zeros_like(x)], axis=2)
    six = Dg.convergence_stats_device(to_iter(x6), thin, warm, layout="iter", detail=True)
    assert np.isnan(six[0][D:]).all() and np.isnan(six[1][D:]).all()
    check((six[0][:D], six[1][:D]), R, neff)
    assert np.array_equal(six[2]["lags_used"][:D], lags)
    assert np.array_equal(six[2]["lags_used"][D:], np.zeros(3, np.int32))
    assert np.array_equal(six[2]["var"][D:], np.zeros(3))
    assert six[2]["passes"] <= three[2]["passes"] + 1


def test_two_calls_agree_bit_for_bit(Dg):
    x, thin, warm, *_ = shape_case("offset")
    d_x = to_iter(x)
    a = Dg.convergence_stats_device(d_x, thin, warm, layout="iter", detail=True)
    b = Dg.convergence_stats_device(d_x, thin, warm, layout="iter", detail=True)
    assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes()
    for k in ("split_mean", "split_sd", "W", "B", "var", "lags_used"):
        assert a[2][k].tobytes() == b[2][k].tobytes(), k
    assert a[2]["passes"] == b[2]["passes"]


def test_lag_block_and_workgroup_options(Dg):
    """8 lags per pass give the bits of 16 (a column's sums do not depend on
    the block of lags they are computed in); another workgroup size reorders
    the sums across chains within the tolerance.  max_lag caps the search."""
    from rhmc_amd import post
    x, thin, warm, R, neff, lags, _ = shape_case("offset")
    d_x = to_iter(x)
    base = Dg.convergence_stats_device(d_x, thin, warm, layout="iter", detail=True)
    c8 = post.PostContext(0, t_blk=8)
    t8 = Dg.convergence_stats_device(d_x, thin, warm, layout="iter", detail=True, ctx=c8)
    assert np.array_equal(t8[0], base[0]) and np.array_equal(t8[1], base[1])
    assert base[2]["passes"] == -(-int(lags.max()) // 16) >= 3
    assert t8[2]["passes"] == -(-int(lags.max()) // 8)
    c8.close()
    x, thin, warm, R, neff, lags, _ = shape_case("c67")
    d_x = to_iter(x)
    base = Dg.convergence_stats_device(d_x, thin, warm, layout="iter", detail=True)
    for block in (64, 128):
        cb = post.PostContext(0, block=block)
        check(Dg.convergence_stats_device(d_x, thin, warm, layout="iter", detail=True, ctx=cb),
              R, neff, lags)
        cb.close()
    cap = Dg.convergence_stats_device(d_x, thin, warm, layout="iter", max_lag=3, detail=True)
    assert np.array_equal(cap[0], base[0])
    assert (cap[2]["lags_used"] <= 3).all() and cap[2]["passes"] == 1
    assert np.isfinite(cap[1]).all()


def test_acceptance(Dg):
    rs = np.random.RandomState(3)
    acc = (rs.rand(61, 67) < 0.7).astype(np.int32)
    dec = acc.T[:, :, None].astype(float)            # the reference's [Nchain][Niter][1]
    d_acc = torch.from_numpy(acc).cuda()
    for kw in (dict(), dict(start=10, end=50)):
        ref = Dg.acceptance_rate(dec, **kw)
        assert np.array_equal(Dg.acceptance_rate_device(d_acc, **kw), ref)
        assert np.array_equal(Dg.acceptance_rate_device(acc, **kw), ref)
    # the asynchronous device-to-device entry on torch's current stream
    from rhmc_amd import post
    rate = torch.empty(67, dtype=torch.float64, device="cuda")
    ctx = post.PostContext(0)
    ctx.acceptance_device(d_acc.data_ptr(), 61, 67, rate.data_ptr(), start=10, end=50,
                          stream=torch.cuda.current_stream().cuda_stream)
    assert np.array_equal(rate.cpu().numpy(), Dg.acceptance_rate(dec, start=10, end=50))
    ctx.close()


class _DeviceOnly:
    """A device array that offers a pointer and a shape, and no way to copy."""

    def __init__(self, t):
        self._t, self.shape, self.dtype, self.device = t, tuple(t.shape), t.dtype, t.device

    def data_ptr(self):
        return self._t.data_ptr()

    def stride(self):
        return self._t.stride()


def test_end_to_end_on_the_engines_record(gpu_lib, Dg):
    """C1, 8 chains, 40 MH iterations of 5 steps with device randoms; the
    record stays in device memory and is read through its pointer."""
    capi = gpu_lib
    from rhmc_amd import workloads
    n_chains, n_iter, n_steps, seed = 8, 40, 5, 2024
    wl = workloads.make("C1", n_chains=n_chains)
    P = capi.make_params(**wl.params)
    ctx = capi.Context(wl.D)
    dev = torch.device("cuda", 0)
    D = wl.q0.shape[1]
    q = torch.from_numpy(np.ascontiguousarray(wl.q0)).to(dev)
    q_chain = torch.zeros((n_iter, n_chains, D), dtype=torch.float64, device=dev)
    accept = torch.zeros((n_iter, n_chains), dtype=torch.int32, device=dev)
    rec = capi.MhRecord(q_chain.data_ptr(), None, None, None, accept.data_ptr())
    ctx.mh_device(P, q.data_ptr(), n_chains, wl.K, n_iter, n_steps, f_pos=True, seed=seed,
                  record=rec)
    ctx.synchronize()
    got = Dg.convergence_stats_device(_DeviceOnly(q_chain), thin_rate=1, warm_up_num=0,
                                      layout="iter", detail=True)
    rate = Dg.acceptance_rate_device(_DeviceOnly(accept))
    rate2 = Dg.acceptance_rate_device(_DeviceOnly(accept), start=10, end=30)
    ctx.close()
    # the host path on a downloaded copy, for comparison only
    x = np.ascontiguousarray(q_chain.cpu().numpy().transpose(1, 0, 2))
    a = accept.cpu().numpy()
    assert 0 < a.mean() <= 1 and np.isfinite(x).all()
    lags, margin = rule_trace(x, 1, 0)
    print("margin %.3e accept %.3f" % (margin, a.mean()))
    assert margin >= MARGIN
    R, neff = Dg.convergence_stats(x, thin_rate=1, warm_up_num=0)
    check(got, R, neff, lags)
    dec = a.T[:, :, None].astype(float)
    assert np.array_equal(rate, Dg.acceptance_rate(dec))
    assert np.array_equal(rate2, Dg.acceptance_rate(dec, start=10, end=30))
