"""CPU checks of RHMC_random (samplers.py:828-1105): the NumPy restatement
tests/rhmc_hess_ref.py against the fixture recorded from the reference
(tests/golden/make_goldens_hess.py), the fixture's own conditions, the host
logic of samplers.lightsource_gym.RHMC_random / RHMC_random_batched with the
context's two calls replaced by the restatement, select_hess(), the C-ABI's
exports, struct and argument errors, and the entry points' error paths under the
host AddressSanitizer."""
import ctypes
import os
import shutil
import subprocess

import numpy as np
import pytest

from conftest import PKG_DIR, ROOT, load_golden
import rhmc_hess_ref

SCENES = rhmc_hess_ref.SCENES
ref_of = rhmc_hess_ref.ref_of


def load_scene(name):
    return rhmc_hess_ref.load_scene(load_golden("rhmc_hess"), name)


def close(got, want, rtol):
    got, want = np.asarray(got, dtype=float), np.asarray(want, dtype=float)
    fin = np.isfinite(want)
    assert got.shape == want.shape
    assert np.array_equal(got[~fin], want[~fin], equal_nan=True)
    assert np.allclose(got[fin], want[fin], rtol=rtol, atol=0.)


def run_args(s):
    return (int(s["n_iter"]), float(s["dt_f"]), float(s["dt_xy"]), float(s["f_lim"]))


@pytest.fixture(scope="module", params=SCENES)
def replay(request):
    s = load_scene(request.param)
    q0 = s["q_model_0"].reshape(-1).copy()
    run = ref_of(s).run(q0, *run_args(s), z=s["z"], steps=s["steps"], lnu=s["lnu"])
    return request.param, s, run, q0


def test_restatement_replays_the_reference(replay):
    """rhmc_hess_ref.run on the recorded draws: A_chain, steps_done, the status
    words and the printed lines exact, the chains and end states to 1e-13 (they
    were recorded from the restatement after it had matched the reference's own
    run to 1e-13); the start array ends as the last row."""
    name, s, run, q0 = replay
    assert np.array_equal(run["A_chain"], s["A_chain"])
    for k in ("q_chain", "E_chain", "dE_chain", "q_end", "p_end", "dE"):
        close(run[k], s[k], 1e-13)
    for k in ("steps_done", "status", "n_run"):
        assert np.array_equal(run[k], s[k]), k
    assert run["lines"] == list(s["lines"])
    assert np.array_equal(q0, run["q_chain"][run["n_run"]], equal_nan=True)


def test_restatement_draws_like_the_reference():
    """From the recorded seed the global stream gives the recorded draws, and
    the next random() after the run is the reference's (also after the early
    stop of `stop`)."""
    for name in ("k3", "stop"):
        s = load_scene(name)
        np.random.seed(int(s["run_seed"]))
        run = ref_of(s).run(s["q_model_0"].reshape(-1).copy(), *run_args(s),
                            int(s["steps_min"]), int(s["steps_max"]))
        for k in ("z", "steps", "lnu"):
            assert np.array_equal(run[k], s[k]), (name, k)
        assert np.random.random() == float(s["next_random"])


def test_fixture_conditions():
    """What make_goldens_hess.py asserted when it wrote the archive."""
    A = []
    for name in SCENES:
        s = load_scene(name)
        n = int(s["n_run"])
        dE, lnu = s["dE"][:n], s["lnu"][:n]
        with np.errstate(invalid="ignore"):
            tested = np.isfinite(dE) & (dE >= 0)
            assert (np.abs(lnu + dE)[tested] >= 1e-3).all(), name
            acc = (dE < 0) | (lnu < -dE)
        assert np.array_equal(acc, s["A_chain"][:n].astype(bool))
        assert not s["A_chain"][n:].any() and not s["q_chain"][n + 1:].any()
        assert s["steps"][:n].min() >= 10 and s["steps"][:n].max() < 50
        assert (s["steps_done"] <= s["steps"]).all()
        assert s["D"].dtype.kind == "u"
        A.append(s["A_chain"][:n])
    A = np.concatenate(A)
    assert A.any() and not A.all()
    w = load_scene("wall")
    broke = (w["steps_done"] < w["steps"]) & (w["steps_done"] > 0)
    assert broke.any() and not np.isfinite(w["dE"]).all() and w["f_lim"] > 0
    assert any("Divergence encountered" in str(ln) for ln in w["lines"])
    st = load_scene("stop")
    assert int(st["n_run"]) == 100 and int(st["n_iter"]) == 120
    assert st["A_chain"][:100].sum() < 50
    for name in SCENES[:3]:
        assert int(load_scene(name)["n_run"]) == 30
    assert os.path.getsize(os.path.join(ROOT, "tests", "golden", "rhmc_hess.npz")) < 256 * 1024


@pytest.mark.parametrize("name", rhmc_hess_ref.FUNCTIONS)
def test_restatement_equals_the_recorded_functions(name):
    """RHMC_efficient_computation's two return forms as recorded from the
    reference, the last state below the wall."""
    s = load_scene(name)
    r = ref_of(s)
    f_lim = float(s["f_lim"])
    n = len(s["q"])
    assert s["q"].shape[1] == 3 * {"fn1": 1, "fn3": 3, "fn10": 10}[name]
    for c in range(n):
        close(r.compute(s["q"][c], s["p"][c], f_lim, dVdqq_only=True), s["dVdqq"][c], 1e-13)
        dqdt, dpdt, E = r.compute(s["q"][c], s["p"][c], f_lim)
        if c == n - 1:
            assert dqdt == dpdt == E == np.inf and s["E"][c] == np.inf
            assert (s["q"][c][0::3] < f_lim).any()
        else:
            close(dqdt, s["dqdt"][c], 1e-13)
            close(dpdt, s["dpdt"][c], 1e-13)
            close(E, s["E"][c], 1e-13)
    (d1, d2, d3, sc) = r.derivs(s["q"][0], scales=True)
    for d, k in zip((d1, d2, d3), sc):
        assert (k >= np.abs(d) * (1 - 1e-12)).all() and (k > 0).all()
    assert np.array_equal(ref_of(s, scale_G=2.).derivs(s["q"][0])[1], 2. * d2)


# ------------------------------------------------------------ the gym's host logic
class RestatementContext:
    """The two calls samplers.lightsource_gym makes for RHMC_random, answered
    by the restatement."""

    def __init__(self, ref, gym):
        self.ref, self.gym = ref, gym
        self.calls = []

    def hess_derivs(self, params, q, V=False):
        q2 = np.asarray(q, dtype=float)
        q2 = q2.reshape(-1, q2.shape[-1])
        self.calls.append(("derivs", q2.shape[0]))
        d = [np.array(x) for x in zip(*[self.ref.derivs(row) for row in q2])]
        Vv = np.array([self.ref.V(row) for row in q2])
        if np.ndim(q) == 1:
            d, Vv = [x[0] for x in d], Vv[0]
        return tuple(d) + ((Vv,) if V else ())

    def hess_random(self, params, dt_f, dt_xy, q, p, steps, derivs=False):
        q2 = np.array(q, dtype=float)
        self.calls.append(("random", q2.shape[0]))
        dt = np.asarray([dt_f, dt_xy, dt_xy] * (q2.shape[1] // 3))
        t = [self.ref.traj(q2[c], np.array(p[c]), int(steps[c]), dt, self.gym.f_lim)
             for c in range(q2.shape[0])]
        out = (q2, np.array([x["p"] for x in t]), np.array([x["status"] for x in t], np.int32),
               np.array([x["steps_done"] for x in t], np.int32))
        if derivs:
            out += tuple(np.array([x["d"][m] for x in t]) for m in range(3))
        return out


def gym_of(s):
    from rhmc_amd.samplers import lightsource_gym
    g = lightsource_gym()
    g.num_rows = g.num_cols = int(s["side"])
    g.B_count, g.PSF_FWHM_pix = float(s["B_count"]), float(s["fwhm_pix"])
    g.D = s["D"].astype(float)
    fake = RestatementContext(ref_of(s), g)
    g._context = lambda: fake
    return g, fake


def sampler_kwargs(s):
    return dict(Niter=int(s["n_iter"]), steps_min=int(s["steps_min"]),
                steps_max=int(s["steps_max"]), f_lim=float(s["f_lim"]),
                dt_RHMC_xy=float(s["dt_xy"]), dt_RHMC_f=float(s["dt_f"]))


@pytest.mark.parametrize("name", SCENES)
def test_gym_RHMC_random_host_logic(name, capsys):
    """Draw order, the unrestored rejection, the overwritten start array, the
    R_accept stop's zero rows and the printed lines, from the recorded seed."""
    s = load_scene(name)
    g, fake = gym_of(s)
    q0 = s["q_model_0"].copy()
    np.random.seed(int(s["run_seed"]))
    g.RHMC_random(q0, debug=True, **sampler_kwargs(s))
    assert np.random.random() == float(s["next_random"])
    n = int(s["n_run"])
    assert capsys.readouterr().out.splitlines() == list(s["lines"])
    assert g.q_chain.shape == (1, int(s["n_iter"]) + 1, q0.size)
    assert g.E_chain.shape == g.dE_chain.shape == (1, int(s["n_iter"]) + 1, 1)
    assert np.array_equal(g.A_chain[0, :, 0], s["A_chain"])
    assert np.array_equal(g.q_chain[0], s["q_chain"], equal_nan=True)
    close(g.E_chain[0, :, 0], s["E_chain"], 1e-13)
    close(g.dE_chain[0, :, 0], s["dE_chain"], 1e-12)
    # not restored after a rejection: every row is its trajectory's end state
    assert np.array_equal(g.q_chain[0, 1:n + 1], s["q_end"][:n], equal_nan=True)
    assert not s["A_chain"][:n].all()
    # the caller's array is overwritten with the last state
    assert np.array_equal(q0.reshape(-1), g.q_chain[0, n], equal_nan=True)
    assert not np.array_equal(q0, s["q_model_0"])
    assert not g.q_chain[0, n + 1:].any() and not g.E_chain[0, n + 1:].any()
    assert g.R_accept == 100. * s["A_chain"].sum() / int(s["n_iter"])
    assert (g.Nobjs, g.d, g.Nchain) == (q0.shape[0], q0.size, 1)
    # one derivative launch at the start, then a trajectory and an energy launch each
    assert fake.calls == [("derivs", 1)] + [("random", 1), ("derivs", 1)] * n


def test_gym_RHMC_efficient_computation_return_shapes():
    s = load_scene("fn3")
    g, _ = gym_of(s)
    g.f_lim = float(s["f_lim"])
    n = len(s["q"])
    for c in range(n):
        h = g.RHMC_efficient_computation(s["q"][c], s["p"][c], debug=False, dVdqq_only=True)
        close(h, s["dVdqq"][c], 1e-13)
        out = g.RHMC_efficient_computation(s["q"][c], s["p"][c])
        if c == n - 1:
            assert out == (np.inf, np.inf, np.inf)
        else:
            for got, key in zip(out, ("dqdt", "dpdt", "E")):
                close(got, s[key][c], 1e-13)


def batched_draws(seed, niter, n, d, steps_min, steps_max):
    """RHMC_random_batched's draws: randn(n, d) in every pass, i = 0 included,
    then randint(size=n) and random(n)."""
    np.random.seed(seed)
    z, steps, lnu = np.zeros((niter + 1, n, d)), np.zeros((niter, n), np.int32), \
        np.zeros((niter, n))
    for i in range(niter + 1):
        z[i] = np.random.randn(n, d)
        if i:
            steps[i - 1] = np.random.randint(low=steps_min, high=steps_max, size=n)
            lnu[i - 1] = np.log(np.random.random(n))
    return z, steps, lnu, np.random.random()


@pytest.mark.parametrize("name", ["k1", "stop"])
def test_gym_batched_with_one_chain_equals_RHMC_random(name, capsys):
    s = load_scene(name)
    g, _ = gym_of(s)
    q0 = s["q_model_0"].reshape(1, -1).copy()
    np.random.seed(int(s["run_seed"]))
    g.RHMC_random_batched(q0, **sampler_kwargs(s))
    nxt = np.random.random()
    assert capsys.readouterr().out == ""
    n = int(s["n_run"])
    assert np.array_equal(g.A_chain[0, :, 0], s["A_chain"])
    assert np.array_equal(g.q_chain[0], s["q_chain"], equal_nan=True)
    close(g.E_chain[0, :, 0], s["E_chain"], 1e-13)
    assert np.array_equal(q0[0], g.q_chain[0, n], equal_nan=True)
    # the stream: the same position unless the chain stopped early, when the
    # batched method draws on to Niter
    want = batched_draws(int(s["run_seed"]), int(s["n_iter"]), 1, q0.size,
                         int(s["steps_min"]), int(s["steps_max"]))[3]
    assert nxt == want
    assert (nxt == float(s["next_random"])) == (name != "stop")


def test_gym_batched_three_chains_against_the_restatement():
    """Three chains of the `stop` scene's image from three starts: chain 0
    stops at i = 100 (its later rows stay zero, its draws are consumed), and
    every chain equals the restatement run on its own columns of the draws."""
    s = load_scene("stop")
    kw = sampler_kwargs(s)
    d = s["q_model_0"].size
    starts = np.stack([s["q_model_0"].reshape(-1),
                       s["q_model_0"].reshape(-1) * np.tile([1.5, 1., 1.], d // 3),
                       s["q_true"].reshape(-1) * np.tile([2., 1., 1.], d // 3)])
    z, steps, lnu, nxt = batched_draws(77, kw["Niter"], 3, d, kw["steps_min"], kw["steps_max"])
    g, fake = gym_of(s)
    q0 = starts.copy()
    np.random.seed(77)
    g.RHMC_random_batched(q0, **kw)
    assert np.random.random() == nxt
    n_run = []
    for c in range(3):
        qc = starts[c].copy()
        run = ref_of(s).run(qc, kw["Niter"], kw["dt_RHMC_f"], kw["dt_RHMC_xy"], kw["f_lim"],
                            z=z[:, c], steps=steps[:, c], lnu=lnu[:, c])
        n_run.append(run["n_run"])
        assert np.array_equal(g.A_chain[c, :, 0], run["A_chain"]), c
        assert np.array_equal(g.q_chain[c], run["q_chain"], equal_nan=True), c
        close(g.E_chain[c, :, 0], run["E_chain"], 1e-13)
        assert np.array_equal(q0[c], qc, equal_nan=True), c
        assert not g.q_chain[c, run["n_run"] + 1:].any()
    assert 100 in n_run, n_run
    # a stopped chain is no longer launched (the one check falls on i = 100)
    assert fake.calls[-1][1] == (sum(n == kw["Niter"] for n in n_run) or 3)


# ---------------------------------------------------------------- selection
def test_select_hess_plans(tmp_path):
    """Every (K, side) in 1..16 x {16, 32, 48} is served with LDS <= 160 KB;
    K = 17 and side 15 are refused (tests/native/hess_select_check.cpp)."""
    gxx = shutil.which("g++")
    if not gxx:
        pytest.skip("g++ not available")
    exe = str(tmp_path / "hess_select_check")
    subprocess.run([gxx, "-std=c++17", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"),
                    "-I", os.path.join(PKG_DIR, "csrc"), "-o", exe,
                    os.path.join(ROOT, "tests", "native", "hess_select_check.cpp")], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "hess select ok" in r.stdout


# -------------------------------------------------------------------- C-ABI
HESS_EXPORTS = ("rhmc_hess_derivs", "rhmc_hess_derivs_device", "rhmc_hess_random",
                "rhmc_hess_random_device")


def test_exports_and_struct():
    from rhmc_amd import capi
    for name in HESS_EXPORTS:
        assert name in capi.EXPORTS and hasattr(capi.lib(), name)
    assert ctypes.sizeof(capi.HessOpts) == 24
    assert capi.HessOpts.dt_f.offset == 0 and capi.HessOpts.dt_xy.offset == 8
    assert capi.HessOpts.reserved.offset == 16 and capi.HessOpts.reserved.size == 8
    assert capi.abi_version() == 4
    hdr = open(os.path.join(ROOT, "include", "rhmc.h")).read()
    assert "#define RHMC_ABI_VERSION 4" in hdr
    for text in ["int %s(rhmc_ctx* ctx" % n for n in HESS_EXPORTS] + \
            ["typedef struct rhmc_hess_opts", "int32_t reserved[2];"]:
        assert text in hdr
    for m in ("hess_derivs", "hess_derivs_device", "hess_random", "hess_random_device"):
        assert hasattr(capi.Context, m)
    from rhmc_amd.samplers import lightsource_gym
    import samplers
    for m in ("RHMC_random", "RHMC_random_batched", "RHMC_efficient_computation"):
        assert hasattr(lightsource_gym, m) and hasattr(samplers.lightsource_gym, m)


def test_bad_arguments_without_a_device():
    """Each bad argument returns a negative code and sets a message (checked
    before the context is touched, so a NULL context serves)."""
    from rhmc_amd import capi
    lib = capi.lib()
    q = np.array([[100., 5., 5.]])
    p = np.zeros((1, 3))
    steps = np.array([10], np.int32)

    def ptr(a):
        return None if a is None else ctypes.c_void_p(a.ctypes.data)

    def call(dt_f=0.1, dt_xy=0.3, reserved=(0, 0), f_lim=0., steps=steps, K=1, n=1, q=q, p=p,
             opts=True, dev=False):
        P = capi.make_params(dt=1., delta=1e-6, counter_max=1000, B_count=25., f_lim=f_lim,
                             f_low=1., fwhm_pix=3.5, g_xx=1., g_ff=1., g_ff2=1., g0=1., g1=1.,
                             g2=1.)
        o = capi.HessOpts(dt_f, dt_xy, (ctypes.c_int32 * 2)(*reserved))
        args = [None, ctypes.byref(P), ctypes.byref(o) if opts else None, ptr(q), ptr(p),
                ptr(steps), n, K, None, None, None, None, None]
        rc = (lib.rhmc_hess_random_device(*args, None) if dev else lib.rhmc_hess_random(*args))
        return rc, lib.rhmc_last_error().decode()

    for dev in (False, True):
        assert call(dev=dev) == (capi.RHMC_ERR_ARG, "ctx is NULL")
        for kw, word in ((dict(steps=None), "steps is NULL"), (dict(opts=False), "opts is NULL"),
                         (dict(q=None), "q/p is NULL"), (dict(p=None), "q/p is NULL"),
                         (dict(dt_f=np.inf), "opts.dt_f"), (dict(dt_f=np.nan), "opts.dt_f"),
                         (dict(dt_xy=-np.inf), "opts.dt_xy"), (dict(dt_xy=np.nan), "opts.dt_xy"),
                         (dict(reserved=(1, 0)), "reserved"), (dict(reserved=(0, 7)), "reserved"),
                         (dict(f_lim=-1.), "f_lim"), (dict(f_lim=-1e-300), "f_lim"),
                         (dict(f_lim=np.nan), "f_lim"), (dict(n=-1), "n_chains < 0"),
                         (dict(K=0), "K must be"), (dict(K=1025), "K must be")):
            rc, msg = call(dev=dev, **kw)
            assert rc == capi.RHMC_ERR_ARG and word in msg, (kw, rc, msg)
    for bad in (0, -3):
        rc, msg = call(steps=np.array([bad], np.int32))
        assert rc == capi.RHMC_ERR_ARG and "steps[i]" in msg
        assert call(steps=np.array([bad], np.int32), dev=True) == (capi.RHMC_ERR_ARG,
                                                                    "ctx is NULL")
    # the derivative sets: no opts, no wall, q alone
    P = capi.make_params(dt=1., delta=1e-6, counter_max=1000, B_count=25., f_lim=-1., f_low=1.,
                         fwhm_pix=3.5, g_xx=1., g_ff=1., g_ff2=1., g0=1., g1=1., g2=1.)
    for dev in (False, True):
        fn = lib.rhmc_hess_derivs_device if dev else lib.rhmc_hess_derivs
        tail = (None,) if dev else ()
        for args, word in (((None, ctypes.byref(P), ptr(q), None, None, None, None, 1, 1),
                            "ctx is NULL"),
                           ((None, None, ptr(q), None, None, None, None, 1, 1), "params is NULL"),
                           ((None, ctypes.byref(P), None, None, None, None, None, 1, 1),
                            "q is NULL"),
                           ((None, ctypes.byref(P), ptr(q), None, None, None, None, -1, 1),
                            "n_chains < 0"),
                           ((None, ctypes.byref(P), ptr(q), None, None, None, None, 1, 0),
                            "K must be")):
            assert fn(*args, *tail) == capi.RHMC_ERR_ARG
            assert word in lib.rhmc_last_error().decode()


def test_hess_error_paths_under_asan():
    """The entry points' argument checks in the host-ASan build of the library
    (tests/native/hess_asan.cpp, a stand-alone program; no device is opened)."""
    exe = os.path.join(ROOT, "build", "asan", "hess_asan")
    if not os.path.exists("/opt/rocm/bin/hipcc"):
        if not os.path.exists(exe):
            pytest.skip("hipcc not available to build the ASan program")
    else:       # (re)build when the sources changed; a no-op otherwise
        subprocess.run(["make", "-C", PKG_DIR, "-j8", "asan-hess"], check=True,
                       capture_output=True)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1")
    r = subprocess.run([exe], capture_output=True, text=True, env=env, timeout=240)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "hess_asan: ok" in r.stdout
    assert "AddressSanitizer" not in r.stderr
