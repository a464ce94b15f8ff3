"""CPU checks of HMC_find_best_dt's step-size search (samplers.py:306-456): the
C-ABI's exports, structs and argument errors, the NumPy restatement
tests/dt_ref.py against the fixture recorded from the reference
(tests/golden/make_goldens_dt.py), the fixture's own conditions, the host part
of the search (samplers.dt_star_search) replayed on the recorded trials, the
kernel-selection rule and the entry points' error paths under the host
AddressSanitizer."""
import ctypes
import os
import shutil
import subprocess

import numpy as np
import pytest

from conftest import PKG_DIR, ROOT, load_golden
import dt_ref

GRADS = ("reference", "full")


def test_exports_structs_and_constants():
    from rhmc_amd import capi
    for name in ("rhmc_dt_trials", "rhmc_dt_trials_device"):
        assert name in capi.EXPORTS and hasattr(capi.lib(), name)
    assert ctypes.sizeof(capi.DtOpts) == 6 * 4
    assert ctypes.sizeof(capi.DtRecord) == 6 * ctypes.sizeof(ctypes.c_void_p)
    assert capi.abi_version() == 4
    hdr = open(os.path.join(ROOT, "include", "rhmc.h")).read()
    assert "RHMC_DT_GRAD_REFERENCE = %d" % capi.DT_GRAD_REFERENCE in hdr
    assert "RHMC_DT_GRAD_FULL = %d" % capi.DT_GRAD_FULL in hdr
    assert "RHMC_OPT_DT_LANES = %d" % capi.OPT_DT_LANES in hdr
    o = capi.make_dt_opts(7, "full", 3, 9)
    assert (o.n_iter, o.grad, o.steps_min, o.steps_max) == (7, capi.DT_GRAD_FULL, 3, 9)
    assert tuple(o.reserved) == (0, 0)
    assert capi.make_dt_opts().grad == capi.DT_GRAD_REFERENCE


def test_bad_arguments_without_a_device():
    """RHMC_ERR_ARG on a NULL context and on bad arguments (checked before the
    context is touched, so no GPU is needed)."""
    from rhmc_amd import capi
    lib = capi.lib()
    P = capi.make_params(dt=1., delta=1e-6, counter_max=1000, B_count=25., f_lim=0., f_low=1.,
                         fwhm_pix=3.5, g_xx=1., g_ff=1., g_ff2=1., g0=1., g1=1., g2=1.)
    bg = np.ones((1, 4, 4))
    bgi = np.zeros(1, np.int32)
    q0 = np.array([[100., 2., 2.]])
    dt = np.array([[1., 0., 0.]])
    z = np.zeros((1, 2, 3))
    steps = np.array([[3, 4]], np.int32)
    lnu = -np.ones((1, 2))
    sid = np.array([5], np.uint64)

    def p(a):
        return None if a is None else ctypes.c_void_p(a.ctypes.data)

    def call(opts, n=1, bg=bg, bgi=bgi, z=z, steps=steps, lnu=lnu, sid=None, dev=False):
        args = [None, ctypes.byref(P), ctypes.byref(opts), p(bg), 1, p(bgi), p(q0), p(dt), None,
                n, p(z), p(steps), p(lnu), ctypes.c_uint64(1), p(sid), None, None]
        if dev:
            return lib.rhmc_dt_trials_device(*args, None)
        return lib.rhmc_dt_trials(*args)

    def err():
        return lib.rhmc_last_error().decode()

    ok = capi.make_dt_opts(2)
    for dev in (False, True):
        assert call(ok, dev=dev) == capi.RHMC_ERR_ARG and "ctx is NULL" in err()
        assert call(ok, z=None, steps=None, lnu=None, sid=sid, dev=dev) == capi.RHMC_ERR_ARG
        assert "ctx is NULL" in err()
    assert call(ok, n=-1) == capi.RHMC_ERR_ARG and "n < 0" in err()
    assert call(ok, bg=None) == capi.RHMC_ERR_ARG and "bg is NULL" in err()
    for n_iter in (0, 1025):
        assert call(capi.make_dt_opts(n_iter)) == capi.RHMC_ERR_ARG and "n_iter" in err()
    assert call(capi.make_dt_opts(2, grad=5)) == capi.RHMC_ERR_ARG and "grad" in err()
    assert call(ok, steps=None) == capi.RHMC_ERR_ARG and "all three or none" in err()
    assert call(ok, z=None, steps=None, lnu=None) == capi.RHMC_ERR_ARG and "stream_id" in err()
    assert call(capi.make_dt_opts(2, steps_min=5, steps_max=5), z=None, steps=None, lnu=None,
                sid=sid) == capi.RHMC_ERR_ARG and "steps_min" in err()
    assert call(ok, bgi=np.array([1], np.int32)) == capi.RHMC_ERR_ARG and "bg_index[0]" in err()
    assert call(ok, steps=np.array([[3, 65536]], np.int32)) == capi.RHMC_ERR_ARG
    assert "steps[1]" in err()
    bad = capi.make_dt_opts(2)
    bad.reserved[1] = 3
    assert call(bad) == capi.RHMC_ERR_ARG and "reserved" in err()


def _gym(s):
    from rhmc_amd.samplers import lightsource_gym
    g = lightsource_gym()
    g.num_rows = g.num_cols = s["side"]
    assert g.B_count == s["B_count"] and g.PSF_FWHM_pix == s["fwhm"]
    return g


@pytest.mark.parametrize("grad", GRADS)
@pytest.mark.parametrize("name", dt_ref.SCENES)
def test_dt_ref_is_pinned_to_the_reference(name, grad):
    """dt_ref's search from the recorded seed, with the package's own
    gen_mock_data drawing the realisations: the reference's final dt bit for
    bit, its stream position, every trial's dt, draws and decisions exactly,
    dE and q of the iterations compared in value to 1e-9."""
    s = dt_ref.load_scene(load_golden("find_best_dt"), name, grad)
    g = _gym(s)
    ref = dt_ref.DtRef(s["D"], s["fwhm"])
    reals, log = [], []

    def gen_mock():
        reals.append(g.gen_mock_data(s["q_model_0"], return_data=True))
        return reals[-1].copy()

    np.random.seed(s["search_seed"])
    dt = dt_ref.search(ref, s["q_model_0"], gen_mock, Niter_per_trial=s["n_iter"], grad=grad,
                       log=log)
    assert np.array_equal(dt, s["dt_final"])
    assert np.random.random() == s["next_random"]
    assert np.array_equal(np.array(reals), s["realisations"])
    assert len(log) == len(s["star"])
    for k in ("star", "phase", "stage"):
        assert np.array_equal([t[k] for t in log], s[k])
    assert np.array_equal(np.array([t["dt"] for t in log]), s["dt"])
    assert np.array_equal(np.array([t["A_rate"] for t in log]), s["A_rate"])
    for k in ("z", "steps", "lnu", "accept"):
        assert np.array_equal(np.array([t[k] for t in log]), s[k]), k
    cmp_ = dt_ref.compared(s["dE"])
    dE = np.array([t["dE"] for t in log])
    assert np.abs(dE - s["dE"])[cmp_].max() <= 1e-9 * (1 + np.abs(s["dE"][cmp_])).max()
    q = np.array([t["q"] for t in log])
    np.testing.assert_allclose(q[cmp_], s["q"][cmp_], rtol=1e-9)


@pytest.mark.parametrize("grad", GRADS)
@pytest.mark.parametrize("name", dt_ref.SCENES)
def test_fixture_conditions(name, grad):
    """What the generator asserted for the reference alone, from the stored
    arrays: margins, the three kinds of iterations, the share compared in
    value; and the records' own consistency."""
    s = dt_ref.load_scene(load_golden("find_best_dt"), name, grad)
    dE, lnu, acc = s["dE"], s["lnu"], s["accept"].astype(bool)
    fin = np.isfinite(dE)
    with np.errstate(invalid="ignore"):
        tested = fin & (dE >= 0)
        margin = np.abs(lnu + dE)
        want = (dE < 0) | (lnu < -dE)
    assert margin[tested].min() >= 1e-3
    assert np.array_equal(acc, want)
    assert acc.any() and (fin & ~acc).any() and (~fin).any()
    assert not acc[~fin].any()
    assert dt_ref.compared(dE).mean() >= 0.6
    assert np.array_equal(s["A_rate"], acc.mean(axis=1))
    assert (lnu <= 0).all() and s["steps"].min() >= 10 and s["steps"].max() < 50
    prev = np.concatenate([s["q0"][:, None, :], s["q"][:, :-1, :]], axis=1)
    assert np.array_equal(s["q"][~acc], prev[~acc])       # a rejection returns to the start
    if grad == "reference":
        n_it = dE.size
        assert 110 <= n_it <= 400 and len(dE) <= 40
    # the flux phase moves the flux alone, whatever the gradient form
    fo = s["flux_only"].astype(bool)
    assert np.array_equal(s["q"][fo][:, :, 1:], np.broadcast_to(
        s["q0"][fo][:, None, 1:], s["q"][fo][:, :, 1:].shape))
    assert (s["dt"][fo][:, 1:] == 0).all() and (s["dt"][~fo][:, 1:] > 0).all()


@pytest.mark.parametrize("grad", GRADS)
@pytest.mark.parametrize("name", dt_ref.SCENES)
def test_host_search_replays_the_recorded_trials(name, grad):
    """samplers.dt_star_search, fed the recorded acceptance counts, asks for
    exactly the recorded trials (phase, stage, dt bit for bit) and returns the
    recorded final dt."""
    from rhmc_amd.samplers import dt_star_search, dt_stream_id
    s = dt_ref.load_scene(load_golden("find_best_dt"), name, grad)
    ids = set()
    for l in range(len(s["q_model_0"])):
        rows = np.flatnonzero(s["star"] == l)
        gen = dt_star_search(l, s["q_model_0"][l, 0], s["n_iter"], 10, 1., 10., 0.9, 0.5)
        req = next(gen)
        last = {}
        for n, r in enumerate(rows):
            k, stage, trial, dt = req
            assert (k, stage) == (s["phase"][r], s["stage"][r])
            assert np.array_equal(dt, s["dt"][r])
            assert trial == last.get((k, stage), -1) + 1       # counted per loop
            last[(k, stage)] = trial
            ids.add(dt_stream_id(l, k, stage, trial))
            try:
                req = gen.send(int(s["accept"][r].sum()))
            except StopIteration as e:
                assert n == len(rows) - 1
                dt_f, dt_xy = e.value
                assert np.array_equal([dt_f, dt_xy, dt_xy], s["dt_final"][3 * l:3 * l + 3])
                break
        else:
            raise AssertionError("the search wants more trials than were recorded")
    assert len(ids) == len(s["star"])                          # one stream per trial


def test_coarse_loop_gives_up_after_64_trials():
    from rhmc_amd.samplers import dt_star_search
    gen = dt_star_search(3, 100., 10, 10, 1., 10., 0.9, 0.5)
    next(gen)
    for _ in range(63):
        gen.send(0)
    with pytest.raises(RuntimeError, match="star 3"):
        gen.send(0)


def test_search_without_rng_still_raises():
    from rhmc_amd.samplers import lightsource_gym
    g = lightsource_gym()
    q = np.array([[1000., 10., 10.]])
    with pytest.raises(NotImplementedError, match="constant background") as e:
        g.HMC_find_best_dt(q_model_0=q, default=False)
    assert 'rng="numpy"' in str(e.value) and 'rng="philox"' in str(e.value)
    with pytest.raises(ValueError):
        g.HMC_find_best_dt(q_model_0=q, default=False, rng="mt")
    g.HMC_find_best_dt(q_model_0=q, default=True, rng="numpy", seed=3)   # read by the search only
    assert np.array_equal(g.dt, [1000., 0.01, 0.01])


def test_select_rule_for_dt_trials(tmp_path):
    gxx = shutil.which("g++")
    if not gxx:
        pytest.skip("g++ not available")
    exe = str(tmp_path / "dt_select_check")
    subprocess.run([gxx, "-std=c++17", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"),
                    "-I", os.path.join(PKG_DIR, "csrc"), "-o", exe,
                    os.path.join(ROOT, "tests", "native", "dt_select_check.cpp")], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "dt select ok" in r.stdout


def test_dt_trials_error_paths_under_asan():
    """The entry points' argument checks in the host-ASan build of the library
    (tests/native/dt_asan.cpp, a stand-alone program; no device is opened)."""
    exe = os.path.join(ROOT, "build", "asan", "dt_asan")
    if not os.path.exists("/opt/rocm/bin/hipcc"):
        if not os.path.exists(exe):
            pytest.skip("hipcc not available to build the ASan program")
    else:       # (re)build when the sources changed; a no-op otherwise
        subprocess.run(["make", "-C", PKG_DIR, "-j8", "asan-dt"], check=True,
                       capture_output=True)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1")
    r = subprocess.run([exe], capture_output=True, text=True, env=env, timeout=240)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "dt_asan: ok" in r.stdout
    assert "AddressSanitizer" not in r.stderr
