"""CPU checks of RHMC_random_diag (samplers.py:668-825): the NumPy restatement
tests/rhmc_diag_ref.py against the fixture recorded from the reference
(tests/golden/make_goldens_diag.py), the fixture's own conditions, the host
methods of samplers.lightsource_gym against the restatement, the C-ABI's
exports, struct and argument errors, and the entry points' error paths under the
host AddressSanitizer."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from conftest import PKG_DIR, ROOT, load_golden
import rhmc_diag_ref

SCENES = rhmc_diag_ref.SCENES
ref_of = rhmc_diag_ref.ref_of


def load_scene(name):
    return rhmc_diag_ref.load_scene(load_golden("rhmc_diag"), name)


def close(got, want, rtol):
    got, want = np.asarray(got, dtype=float), np.asarray(want, dtype=float)
    fin = np.isfinite(want)
    assert got.shape == want.shape
    assert np.array_equal(got[~fin], want[~fin], equal_nan=True)
    assert np.allclose(got[fin], want[fin], rtol=rtol, atol=0.)


@pytest.fixture(scope="module", params=SCENES)
def replay(request):
    s = load_scene(request.param)
    run = ref_of(s).run(s["q_model_0"].reshape(-1), int(s["n_iter"]), float(s["dt_global"]),
                        float(s["f_lim"]), z=s["z"], steps=s["steps"], lnu=s["lnu"],
                        save_traj="qs" in s)
    return request.param, s, run


def test_restatement_replays_the_reference(replay):
    """rhmc_diag_ref.run on the recorded draws: A_chain exact, q_chain and
    E_chain to 1e-13 (they were recorded from the restatement after it had
    matched the reference's own run to 1e-13)."""
    name, s, run = replay
    assert np.array_equal(run["A_chain"], s["A_chain"])
    close(run["q_chain"], s["q_chain"], 1e-13)
    close(run["E_chain"], s["E_chain"], 1e-13)
    close(run["q_end"], s["q_end"], 1e-13)
    close(run["p_end"], s["p_end"], 1e-13)
    assert np.array_equal(run["flipped_last"], s["flipped_last"])
    if "qs" in s:
        for i, n in enumerate(s["traj_len"]):
            close(run["qs"][i], s["qs"][i, :n], 1e-13)
            close(run["Vs"][i], s["Vs"][i, :n], 1e-13)
            close(run["Ts"][i], s["Ts"][i, :n], 1e-13)
            assert np.isnan(s["Vs"][i, n:]).all()


def test_restatement_draws_like_the_reference():
    """From the recorded seed the global stream gives the recorded draws, and
    the next random() after the run is the reference's."""
    s = load_scene("k3")
    np.random.seed(int(s["run_seed"]))
    run = ref_of(s).run(s["q_model_0"].reshape(-1), int(s["n_iter"]), float(s["dt_global"]),
                        float(s["f_lim"]), int(s["steps_min"]), int(s["steps_max"]))
    assert np.array_equal(run["z"], s["z"]) and np.array_equal(run["steps"], s["steps"])
    assert np.array_equal(run["lnu"], s["lnu"])
    assert np.random.random() == float(s["next_random"])


def test_fixture_conditions():
    """What make_goldens_diag.py asserted when it wrote the archive."""
    A = []
    for name in SCENES:
        s = load_scene(name)
        dE, lnu = s["dE"], s["lnu"]
        with np.errstate(invalid="ignore"):
            tested = np.isfinite(dE) & (dE >= 0)
            assert (np.abs(lnu + dE)[tested] >= 1e-3).all(), name
            acc = (dE < 0) | (lnu < -dE)
        assert np.array_equal(acc, s["A_chain"].astype(bool))
        assert s["steps"].min() >= 10 and s["steps"].max() < 50 and len(dE) == 40
        assert s["D"].dtype.kind == "u"
        A.append(s["A_chain"])
    A = np.concatenate(A)
    assert A.any() and not A.all()
    w = load_scene("wall")
    assert w["flipped_last"].any() and not np.isfinite(w["dE"]).all() and w["f_lim"] > 0
    assert os.path.getsize(os.path.join(ROOT, "tests", "golden", "rhmc_diag.npz")) < 256 * 1024


@pytest.mark.parametrize("name", ["k1", "k3", "wall"])
def test_gym_host_methods_equal_the_restatement(name):
    """mass_matrix, F, G, dlnDetdq, dpMpdq, K(p, M) and compute_factors are
    host methods: no GPU."""
    from rhmc_amd.samplers import lightsource_gym
    s = load_scene(name)
    r = ref_of(s)
    g = lightsource_gym()
    g.num_rows = g.num_cols = int(s["side"])
    assert g.factor1 is None
    g.compute_factors()
    assert g.factor1 == float(s["factor1"]) == rhmc_diag_ref.factor1_of(
        g.num_rows, g.num_cols, g.PSF_FWHM_pix)
    assert g.factor0 > 0 and g.factor2 > 0
    for i in (0, 7, 23, 39):
        q, pe = s["q_end"][i], s["p_end"][i]
        if not np.isfinite(q).all():
            continue
        M = g.mass_matrix(q)
        assert np.array_equal(M, r.mass_matrix(q))
        assert np.array_equal(g.dlnDetdq(q), r.dlnDetdq(q))
        assert np.array_equal(g.dpMpdq(q, pe), r.dpMpdq(q, pe))
        assert g.K(pe, M) == r.K(pe, M)
        assert g.K(pe) == np.dot(pe, pe) / 2.
        assert np.array_equal(g._mass_batch(q[None])[0], M)
        assert np.allclose(g._K_batch(pe[None], M[None])[0], r.K(pe, M), rtol=1e-15, atol=0.)
        f = q[0]
        assert g.F(f) == f * g.factor1 and g.F(f, dFdf=True) == (f * g.factor1, g.factor1)
        assert g.G(f) == 1. / f and g.G(f, dGdf=True) == (1. / f, -1 / f ** 2)


def test_log_determinant_is_the_log_of_a_running_product():
    """K overflows where the reference's does (prod first, then one log)."""
    from rhmc_amd.samplers import lightsource_gym
    g = lightsource_gym()
    M = np.full(60, 1e6)
    with np.errstate(over="ignore"):
        assert g.K(np.zeros(60), M) == np.inf
        assert g._K_batch(np.zeros((1, 60)), M[None])[0] == np.inf


def test_exports_and_struct():
    from rhmc_amd import capi
    for name in ("rhmc_diag_random", "rhmc_diag_random_device"):
        assert name in capi.EXPORTS and hasattr(capi.lib(), name)
    assert ctypes.sizeof(capi.DiagOpts) == 24
    assert capi.abi_version() == 4
    hdr = open(os.path.join(ROOT, "include", "rhmc.h")).read()
    assert "#define RHMC_ABI_VERSION 4" in hdr
    for text in ("int rhmc_diag_random(rhmc_ctx* ctx", "int rhmc_diag_random_device(rhmc_ctx* ctx",
                 "typedef struct rhmc_diag_opts"):
        assert text in hdr
    assert hasattr(capi.Context, "diag_random") and hasattr(capi.Context, "diag_random_device")


def test_bad_arguments_without_a_device():
    """Each bad argument returns a negative code and sets a message (checked
    before the context is touched, so a NULL context serves)."""
    from rhmc_amd import capi
    lib = capi.lib()
    P = capi.make_params(dt=1., delta=1e-6, counter_max=1000, B_count=25., f_lim=0., f_low=1.,
                         fwhm_pix=3.5, g_xx=1., g_ff=1., g_ff2=1., g0=1., g1=1., g2=1.)
    q = np.array([[100., 5., 5.]])
    p = np.zeros((1, 3))
    steps = np.array([10], np.int32)
    trace = np.zeros((1, 11, 3))

    def ptr(a):
        return None if a is None else ctypes.c_void_p(a.ctypes.data)

    def call(dt=1e-2, f1=0.45, rows=11, steps=steps, K=1, trace=None, opts=True, dev=False):
        o = capi.DiagOpts(dt, f1, rows, 0)
        args = [None, ctypes.byref(P), ctypes.byref(o) if opts else None, ptr(q), ptr(p),
                ptr(steps), 1, K, None, ptr(trace)]
        rc = (lib.rhmc_diag_random_device(*args, None) if dev else lib.rhmc_diag_random(*args))
        return rc, lib.rhmc_last_error().decode()

    for dev in (False, True):
        assert call(dev=dev) == (capi.RHMC_ERR_ARG, "ctx is NULL")
        for kw, word in ((dict(steps=None), "steps is NULL"), (dict(opts=False), "opts is NULL"),
                         (dict(f1=0.), "factor1"), (dict(f1=-1.), "factor1"),
                         (dict(f1=np.inf), "factor1"), (dict(f1=np.nan), "factor1"),
                         (dict(dt=np.inf), "opts.dt"), (dict(dt=np.nan), "opts.dt"),
                         (dict(K=0), "K must be"), (dict(K=1025), "K must be"),
                         (dict(trace=trace, rows=1), "trace_rows")):
            rc, msg = call(dev=dev, **kw)
            assert rc < 0 and word in msg, (kw, rc, msg)
    rc, msg = call(trace=trace, rows=10)                # 10 steps need 11 rows
    assert rc == capi.RHMC_ERR_ARG and "trace_rows = 10" in msg
    assert call(trace=trace, rows=11) == (capi.RHMC_ERR_ARG, "ctx is NULL")
    rc, msg = call(steps=np.array([0], np.int32))
    assert rc == capi.RHMC_ERR_ARG and "steps[i]" in msg


def test_diag_random_error_paths_under_asan():
    """The entry points' argument checks in the host-ASan build of the library
    (tests/native/diag_asan.cpp, a stand-alone program; no device is opened)."""
    exe = os.path.join(ROOT, "build", "asan", "diag_asan")
    if not os.path.exists("/opt/rocm/bin/hipcc"):
        if not os.path.exists(exe):
            pytest.skip("hipcc not available to build the ASan program")
    else:       # (re)build when the sources changed; a no-op otherwise
        subprocess.run(["make", "-C", PKG_DIR, "-j8", "asan-diag"], check=True,
                       capture_output=True)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1")
    r = subprocess.run([exe], capture_output=True, text=True, env=env, timeout=240)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "diag_asan: ok" in r.stdout
    assert "AddressSanitizer" not in r.stderr
