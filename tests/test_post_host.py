"""CPU-only checks of librhmc_post.so (include/rhmc_post.h): it loads without
a GPU, exports what the header declares, its structs match the header, every
argument error is reported before any HIP call, and the host-only stopping
rule rhmc_post_neff reproduces the reference's n_eff on NumPy-computed
variograms of the golden chains."""
import ctypes
import os
import re

import numpy as np
import pytest

from conftest import ROOT, load_golden

ERR_ARG = -1


def _header():
    return open(os.path.join(ROOT, "include", "rhmc_post.h")).read()


def _header_functions():
    return sorted(set(re.findall(r"\b(rhmc_post_[a-z_]+)\s*\(", _header())))


@pytest.fixture(scope="module")
def P():
    from rhmc_amd import post
    return post


def test_library_loads_and_exports_every_declared_symbol(P):
    declared = _header_functions()
    assert len(declared) >= 10, declared
    missing = [s for s in declared if not hasattr(P.lib(), s)]
    assert not missing, missing
    assert sorted(P.EXPORTS) == declared
    for name in ("rhmc_post_abi_version", "rhmc_post_last_error", "rhmc_post_create",
                 "rhmc_post_destroy", "rhmc_post_convergence_device", "rhmc_post_convergence",
                 "rhmc_post_variogram_device", "rhmc_post_neff", "rhmc_post_acceptance_device",
                 "rhmc_post_acceptance"):
        assert name in declared, name


def test_package_does_not_import_the_binding():
    import subprocess
    import sys
    from conftest import PKG_DIR
    code = ("import sys; sys.path.insert(0, %r); import rhmc_amd, rhmc_amd.diagnostics; "
            "assert 'rhmc_amd.post' not in sys.modules" % PKG_DIR)
    subprocess.run([sys.executable, "-c", code], check=True)


def test_abi_version_and_struct_layout(P):
    assert P.abi_version() == P.ABI_VERSION == 1
    assert int(re.search(r"#define RHMC_POST_ABI_VERSION (\d+)", _header()).group(1)) == 1
    # the header's structs: 5 int64; 8 pointers + 2 int32
    lay = re.search(r"typedef struct rhmc_post_layout \{(.*?)\}", _header(), re.S).group(1)
    assert len(re.findall(r"\bint64_t\s+\w+;", lay)) == 5
    assert ctypes.sizeof(P.PostLayout) == 5 * 8
    det = re.search(r"typedef struct rhmc_post_detail \{(.*?)\} rhmc_post_detail", _header(),
                    re.S).group(1)
    det = re.sub(r"/\*.*?\*/", "", det, flags=re.S)
    fields = re.findall(r"(\*?)\s*(\w+);", det)
    assert [f[1] for f in fields] == [n for n, _ in P.PostDetail._fields_]
    assert sum(1 for f in fields if f[0]) == 8
    assert ctypes.sizeof(P.PostDetail) == 8 * 8 + 2 * 4


def _conv(P, ctx=None, x=1, n_iter=40, n_chains=4, D=3, ld_iter=None, ld_chain=None, warm=0,
          thin=1, max_lag=0, R=1, neff=1, device=True, null_layout=False):
    """A call with fake non-NULL pointers: it must fail before touching them."""
    lay = P.make_layout(n_iter, n_chains, D, ld_iter, ld_chain)
    buf = np.zeros(max(D, 1))
    args = [ctypes.c_void_p(ctx), ctypes.c_void_p(0x1000 if x else 0),
            None if null_layout else ctypes.byref(lay), warm, thin, max_lag,
            buf.ctypes.data if R else None, buf.ctypes.data if neff else None, None]
    if device:
        return P.lib().rhmc_post_convergence_device(*args, None)
    return P.lib().rhmc_post_convergence(*args)


@pytest.mark.parametrize("device", [True, False])
@pytest.mark.parametrize("kw,word", [
    (dict(n_chains=1), "n_chains"),
    (dict(D=0), "D must"),
    (dict(thin=0), "thin"),
    (dict(warm=-1), "warm_up"),
    (dict(n_iter=5), "n = 2"),              # n = 2 < 3
    (dict(n_iter=40, warm=36), "n = 2"),
    (dict(n_iter=40, thin=8), "n = 2"),     # 5 kept rows
    (dict(warm=50), "n = 0"),
    (dict(ld_iter=-12), "stride"),
    (dict(ld_chain=-3, ld_iter=12), "stride"),
    (dict(max_lag=-1), "max_lag"),
    (dict(null_layout=True), "layout"),
    (dict(), "NULL"),                       # everything valid but ctx
    (dict(ctx=0x1000, x=0), "NULL"),
    (dict(ctx=0x1000, R=0), "NULL"),
    (dict(ctx=0x1000, neff=0), "NULL"),
])
def test_convergence_argument_errors_need_no_gpu(P, kw, word, device):
    rc = _conv(P, device=device, **kw)
    assert rc == ERR_ARG
    assert word in P.last_error(), P.last_error()


def test_other_argument_errors_need_no_gpu(P):
    L = P.lib()
    lay = P.make_layout(40, 4, 3)
    V = np.zeros(64)
    fake = ctypes.c_void_p(0x1000)
    vg = L.rhmc_post_variogram_device
    assert vg(None, fake, ctypes.byref(lay), 0, 1, 1, 4, V.ctypes.data, None) == ERR_ARG
    assert "NULL" in P.last_error()
    for lag0, n_lags in ((0, 1), (1, 0), (20, 1), (1, 20), (19, 2)):   # n = 20: lags 1 .. 19
        assert vg(fake, fake, ctypes.byref(lay), 0, 1, lag0, n_lags, V.ctypes.data,
                  None) == ERR_ARG
        assert "lags" in P.last_error()
    bad = P.make_layout(40, 1, 3)
    assert vg(fake, fake, ctypes.byref(bad), 0, 1, 1, 1, V.ctypes.data, None) == ERR_ARG
    assert "n_chains" in P.last_error()
    acc = (L.rhmc_post_acceptance_device, L.rhmc_post_acceptance_fetch)
    for fn in acc:
        for start, end in ((-1, 5), (0, -1), (5, 5), (6, 5), (0, 41), (-2, -2), (-3, 10)):
            assert fn(fake, fake, 40, 4, 4, start, end, fake, None) == ERR_ARG
            assert "start" in P.last_error()
        assert fn(fake, fake, 0, 4, 4, -1, -1, fake, None) == ERR_ARG
        assert fn(fake, fake, 40, 0, 4, -1, -1, fake, None) == ERR_ARG
        assert fn(fake, fake, 40, 4, -4, -1, -1, fake, None) == ERR_ARG
        assert "stride" in P.last_error()
        assert fn(None, fake, 40, 4, 4, -1, -1, fake, None) == ERR_ARG
        assert fn(fake, None, 40, 4, 4, 10, 20, fake, None) == ERR_ARG
        assert fn(fake, fake, 40, 4, 4, -1, -1, None, None) == ERR_ARG
        assert "NULL" in P.last_error()
    assert L.rhmc_post_acceptance(fake, fake, 40, 4, 4, 5, 5, fake) == ERR_ARG
    assert L.rhmc_post_acceptance(None, fake, 40, 4, 4, -1, -1, fake) == ERR_ARG
    assert L.rhmc_post_create(0, None) == ERR_ARG
    h = ctypes.c_void_p()
    assert L.rhmc_post_create(-1, ctypes.byref(h)) == ERR_ARG and not h.value
    assert L.rhmc_post_set_option(None, P.OPT_TBLK, 7) == ERR_ARG
    assert L.rhmc_post_set_option(None, P.OPT_TBLK, 8) == ERR_ARG
    assert L.rhmc_post_set_option(fake, 99, 8) == ERR_ARG
    out, dec = ctypes.c_double(), ctypes.c_int32()
    nf = L.rhmc_post_neff
    assert nf(1, 10, 1., V.ctypes.data, 4, ctypes.byref(out), ctypes.byref(dec)) == ERR_ARG
    assert nf(4, 2, 1., V.ctypes.data, 4, ctypes.byref(out), ctypes.byref(dec)) == ERR_ARG
    assert nf(4, 10, 1., None, 4, ctypes.byref(out), ctypes.byref(dec)) == ERR_ARG
    assert nf(4, 10, 1., V.ctypes.data, 4, None, ctypes.byref(dec)) == ERR_ARG
    assert nf(4, 10, 1., V.ctypes.data, -1, ctypes.byref(out), ctypes.byref(dec)) == ERR_ARG
    L.rhmc_post_destroy(None)   # a no-op


def _split(x, thin, warm):
    """convergence_stats's split sequences [m][n][D] and its pooled var."""
    chains = []
    for c in x:
        c = c[warm:][::thin]
        L = c.shape[0] - c.shape[0] % 2
        chains += [c[:L // 2], c[L // 2:L]]
    y = np.array(chains)
    m, n, _ = y.shape
    W = np.mean(np.std(y, ddof=1, axis=1), axis=0)
    mw = np.mean(y, axis=1)
    B = np.sum(np.square(mw - np.mean(mw, axis=0)), axis=0) * n / float(m - 1)
    return y, W * (n - 1) / float(n) + B / float(n)


def _variograms(y, d):
    m, n, _ = y.shape
    return np.array([np.sum(np.square(y[:, t:, d] - y[:, :-t, d])) / float(m * (n - t))
                     for t in range(1, n)])


@pytest.mark.parametrize("name", ["iid", "ar", "ar_hi"])
@pytest.mark.parametrize("thin,warm,key", [(2, 10, "neff"), (1, 0, "neff1")])
def test_neff_rule_reproduces_the_reference(P, name, thin, warm, key):
    z = load_golden("solvers")
    x = z["conv_" + name + "/x"]
    gold = z["conv_" + name + "/" + key]
    y, var = _split(x, thin, warm)
    m, n, D = y.shape
    for d in range(D):
        V = _variograms(y, d)
        ne, decided = P.neff(m, n, var[d], V)
        assert decided == 1
        np.testing.assert_allclose(ne, gold[d], rtol=1e-13)
        # the shortest lag list that decides: one lag fewer must report 0
        # (where the rule needs more than V_1), one more changes nothing
        need = next(k for k in range(1, n) if P.neff(m, n, var[d], V[:k])[1] == 1)
        assert P.neff(m, n, var[d], V[:need])[0] == ne
        rho1 = 1. - V[0] / (2. * var[d])
        if rho1 < 0.05:
            assert need == 1 and ne == m * n
        else:
            assert need >= 3
            part, dec = P.neff(m, n, var[d], V[:need - 1])
            assert dec == 0 and np.isfinite(part)
            assert P.neff(m, n, var[d], V[:0]) == (float(m * n), 0)


def test_neff_rule_edges(P):
    # n = 3: rho_1 alone; t = n - 2 = 1 without a loop
    ne, dec = P.neff(4, 3, 1., [0.5])
    assert dec == 1 and ne == 12 / (1 + 2 * 0.75)
    # degenerate variance: NaN, decided, no lags needed
    for var in (0., -1., np.nan, np.inf):
        ne, dec = P.neff(4, 10, var, [])
        assert dec == 1 and np.isnan(ne)
    # exhaustion: slowly decaying positive rho never fires; every lag is summed to n - 2
    n = 12
    rho = np.linspace(0.9, 0.1, n - 1)
    V = 2. * (1. - rho)
    ne, dec = P.neff(6, n, 1., V)
    assert dec == 1
    np.testing.assert_allclose(ne, 6 * n / (1 + 2 * np.sum(rho[:n - 2])), rtol=1e-14)
    assert P.neff(6, n, 1., V[:n - 2])[1] == 0
    # the rule fires at t = 1: only rho_1 is summed
    ne, dec = P.neff(4, 10, 1., 2. * (1. - np.array([0.06, -0.5, -0.5, 0.9])))
    assert dec == 1
    np.testing.assert_allclose(ne, 40 / (1 + 2 * 0.06), rtol=1e-14)
