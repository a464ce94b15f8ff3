"""GPU parity of find_peaks' seed descent (rhmc_find_peaks; samplers.py:129-254)
against the fixture recorded from the reference's own find_peaks
(tests/golden/make_goldens_peaks.py) and against tests/peaks_ref.py, on the
one-launch kernel (peaks_k1_tiledr) and on the stepwise path.

Bar, for every seed that is not exempt: steps and status exactly the
reference's; final (f, x, y) within 1e-9 relative to |value| + 1 (the descent
contracts, errors do not grow); final V within 1e-10 relative.

Exemption.  The convergence test compares |dV/V| with 1e-9, and the
reference's own ratio carries np.sum's rounding: re-evaluating it with
math.fsum moved it by up to `noise` (2.4e-7 ... 4.4e-7 of the threshold,
measured by the generator per case over every step within a factor 2 of the
threshold).  A seed is exempt from the exact-count rule only if the
reference's ratio came within 10 x noise of the threshold at some step, or its
flux within 1e-9 relative of f_lim; it must still stop for the same reason
within +-1 step, at the state peaks_ref reaches with that many forced steps
(1e-9).  At most 5 % of a case's seeds may be exempt (none of the fixture's
is: the closest ratios are 9.4e-4 / 2.2e-5 / 8.7e-4 of the threshold).  For
inputs that are not in the fixture the band is 10 x the largest noise of the
fixture's cases, and the margins come from peaks_ref's trace.
"""
import numpy as np
import pytest

from conftest import load_golden
import peaks_ref

pytestmark = pytest.mark.gpu

CASES = ["A", "A60", "B", "C"]
REASON_NAMES = ["converged", "faint", "cap"]        # the fixture's reason codes 0, 1, 2
_cache = {}


def _codes(capi):
    return {"converged": capi.PEAK_CONVERGED, "faint": capi.PEAK_FAINT, "cap": capi.PEAK_CAP}


def _params(capi, B_count, fwhm_pix):
    return capi.make_params(dt=1., delta=1e-6, counter_max=1000, B_count=B_count, f_lim=0.,
                            f_low=1., fwhm_pix=fwhm_pix, g_xx=1., g_ff=1., g_ff2=1., g0=1.,
                            g1=1., g2=1.)


def _golden():
    if "z" not in _cache:
        _cache["z"] = load_golden("find_peaks")
    return _cache["z"]


def _band_default():
    z = _golden()
    return 10 * max(float(z[c + "/noise"]) for c in CASES)


def _want_golden(name):
    z = _golden()
    return dict(q=z[name + "/q_final"], steps=z[name + "/steps"],
                reasons=[REASON_NAMES[r] for r in z[name + "/reason"]], V=z[name + "/V_final"],
                ratio_margin=z[name + "/ratio_margin"], f_margin=z[name + "/f_margin"],
                band=10 * float(z[name + "/noise"]))


def _want_ref(key, D, B_count, fwhm_pix, seeds, f_lim, n_step):
    """peaks_ref on `seeds`, with the exemption margins from its trace (once per key)."""
    if key in _cache:
        return _cache[key]
    ref = peaks_ref.PeaksRef(D, B_count, fwhm_pix)
    n = len(seeds)
    w = dict(q=np.zeros((n, 3)), steps=np.zeros(n, np.int64), reasons=[], V=np.zeros(n),
             ratio_margin=np.full(n, np.inf), f_margin=np.full(n, np.inf),
             band=_band_default())
    for i, s in enumerate(seeds):
        tr = []
        f, x, y, st, why, V = ref.descend(s, f_lim, n_step=n_step, trace=tr)
        w["q"][i] = (f, x, y)
        w["steps"][i] = st
        w["reasons"].append(why)
        w["V"][i] = V
        for ratio, fl in tr:
            if ratio is not None and np.isfinite(ratio):
                w["ratio_margin"][i] = min(w["ratio_margin"][i], abs(ratio - 1e-9) / 1e-9)
            if np.isfinite(fl):
                w["f_margin"][i] = min(w["f_margin"][i], abs(fl - f_lim) / f_lim)
    _cache[key] = w
    return w


def _run(capi, D, B_count, fwhm_pix, seeds, f_lim, n_step, fused=True, kernel=None):
    ctx = capi.Context(D, device=0, kernel=kernel)
    ctx.set_option(capi.OPT_PEAKS_FUSED, int(fused))
    try:
        return ctx.find_peaks(_params(capi, B_count, fwhm_pix),
                              capi.make_peaks_opts(f_lim, n_step=n_step), seeds)
    finally:
        ctx.close()


def _run_case(capi, name, fused):
    key = ("gpu", name, fused)
    if key not in _cache:
        z = _golden()
        _cache[key] = _run(capi, z[name + "/D"], float(z[name + "/B_count"]),
                           float(z[name + "/fwhm_pix"]), z[name + "/grid"],
                           float(z[name + "/f_lim"]), int(z[name + "/Nstep"]), fused=fused)
    return _cache[key]


def _check(capi, got, want, label, ref=None, seeds=None, f_lim=None):
    """The module docstring's bar.  ref / seeds / f_lim: for the forced-steps
    comparison of exempt seeds."""
    q, steps, status, V = got
    codes = _codes(capi)
    n = len(steps)
    exempt = (want["ratio_margin"] < want["band"]) | (want["f_margin"] < 1e-9)
    print("%s: %d of %d seeds exempt (band %.3g)" % (label, exempt.sum(), n, want["band"]))
    assert exempt.sum() <= 0.05 * n
    for i in range(n):
        code = codes[want["reasons"][i]]
        if not np.all(np.isfinite(want["q"][i])):
            code |= capi.STATUS_NONFINITE
        assert status[i] == code, (label, i, status[i], want["reasons"][i])
        if exempt[i]:
            assert abs(int(steps[i]) - int(want["steps"][i])) <= 1, (label, i)
            f, x, y = ref.descend(seeds[i], f_lim, force_steps=int(steps[i]))[:3]
            wq = np.array([f, x, y])
        else:
            assert steps[i] == want["steps"][i], (label, i, steps[i], want["steps"][i])
            wq = want["q"][i]
            assert abs(V[i] - want["V"][i]) <= 1e-10 * abs(want["V"][i]), (label, i)
        err = np.abs(q[i] - wq) / (np.abs(wq) + 1)
        assert err.max() <= 1e-9, (label, i, q[i], wq)


def _ref_of(name):
    z = _golden()
    return (peaks_ref.PeaksRef(z[name + "/D"], float(z[name + "/B_count"]),
                               float(z[name + "/fwhm_pix"])),
            z[name + "/grid"], float(z[name + "/f_lim"]))


@pytest.mark.parametrize("fused", [True, False], ids=["fused", "stepwise"])
@pytest.mark.parametrize("name", CASES)
def test_descent_matches_reference(gpu_lib, name, fused):
    """A / A60 / B / C: every seed's steps, stop reason, state and V."""
    ref, grid, f_lim = _ref_of(name)
    _check(gpu_lib, _run_case(gpu_lib, name, fused), _want_golden(name),
           "%s %s" % (name, "fused" if fused else "stepwise"), ref, grid, f_lim)


@pytest.mark.parametrize("name", CASES)
def test_fused_and_stepwise_agree(gpu_lib, name):
    """The two paths against each other, same rule (A60: the cap, and waves
    whose seeds stop at different steps)."""
    capi = gpu_lib
    qa, sa, ta, Va = _run_case(capi, name, True)
    qb, sb, tb, Vb = _run_case(capi, name, False)
    w = _want_golden(name)
    exempt = (w["ratio_margin"] < w["band"]) | (w["f_margin"] < 1e-9)
    print("%s fused vs stepwise: %d seeds exempt" % (name, exempt.sum()))
    assert np.array_equal(ta, tb)
    assert np.all(np.abs(sa - sb)[exempt] <= 1) and np.array_equal(sa[~exempt], sb[~exempt])
    same = sa == sb
    assert (np.abs(qa - qb) / (np.abs(qb) + 1))[same].max() <= 1e-9
    assert np.all(np.abs(Va - Vb)[same] <= 1e-10 * np.abs(Vb)[same])
    if name == "A60":
        assert len(set(sa.tolist())) > 2 and (ta == capi.PEAK_CAP).any()


def test_ragged_batches_and_permutation(gpu_lib):
    """A's 49 seeds are a ragged last wave; n = 1, 3, 5 and a permutation of A
    change nothing per seed (steps and status exactly, states to 1e-12: a
    seed's last bits may follow its wave-mates' PSF-factor path), and two
    identical calls are bit-identical."""
    capi = gpu_lib
    z = _golden()
    D, grid = z["A/D"], z["A/grid"]
    args = (float(z["A/B_count"]), float(z["A/fwhm_pix"]))
    f_lim, n_step = float(z["A/f_lim"]), int(z["A/Nstep"])
    q, s, t, V = _run_case(capi, "A", True)
    q2, s2, t2, V2 = _run(capi, D, *args, grid, f_lim, n_step)
    assert np.array_equal(q, q2) and np.array_equal(s, s2) and np.array_equal(t, t2)
    assert np.array_equal(V, V2)
    perm = np.random.RandomState(1).permutation(len(grid))
    for idx in (np.arange(1), np.arange(3), np.arange(5), perm):
        qs, ss, ts, Vs = _run(capi, D, *args, grid[idx], f_lim, n_step)
        assert np.array_equal(ss, s[idx]) and np.array_equal(ts, t[idx]), len(idx)
        assert (np.abs(qs - q[idx]) / (np.abs(q[idx]) + 1)).max() <= 1e-12
        assert np.all(np.abs(Vs - V[idx]) <= 1e-12 * np.abs(V[idx]))


def test_fp64_pixel_cache(gpu_lib):
    """Case A with D + 0.25 (not exact in fp32: the fp64 image cache) vs peaks_ref."""
    capi = gpu_lib
    z = _golden()
    D = z["A/D"] + 0.25
    B, fw, f_lim = float(z["A/B_count"]), float(z["A/fwhm_pix"]), float(z["A/f_lim"])
    grid = z["A/grid"][::2]
    n_step = 1000
    want = _want_ref("f64", D, B, fw, grid, f_lim, n_step)
    got = _run(capi, D, B, fw, grid, f_lim, n_step)
    _check(capi, got, want, "A + 0.25", peaks_ref.PeaksRef(D, B, fw), grid, f_lim)


def test_edge_far_faint_and_nan_seeds(gpu_lib):
    """32 px: seeds at x = 0.3 and x = 31.8 (clamped windows), at (-3, 10),
    at (10, 52) (the PSF misses the image: dV = 0, CONVERGED at step 1 with
    the state unchanged), one that is faint after its first step, and a NaN
    seed (CAP | NONFINITE, steps = n_step) whose three wave-mates are unaffected."""
    capi = gpu_lib
    z = _golden()
    D, grid = z["A/D"], z["A/grid"]
    B, fw, f_lim = float(z["A/B_count"]), float(z["A/fwhm_pix"]), float(z["A/f_lim"])
    fs = float(z["A/f_seed"])
    n_step = 120
    faint0 = z["A/q_final"][np.flatnonzero(z["A/reason"] == 1)[0]]
    seeds = np.array([grid[0], [np.nan, 10., 10.], grid[1], grid[2],
                      [fs, 0.3, 10.], [fs, 31.8, 20.], [fs, -3., 10.], [fs, 10., 52.], faint0])
    fin = np.array([i for i in range(len(seeds)) if i != 1])
    want = _want_ref("edge", D, B, fw, seeds[fin], f_lim, n_step)
    assert want["reasons"][6] == "converged" and want["steps"][6] == 1
    assert want["reasons"][7] == "faint" and want["steps"][7] == 1
    for fused in (True, False):
        q, s, t, V = _run(capi, D, B, fw, seeds, f_lim, n_step, fused=fused)
        assert t[1] == capi.PEAK_CAP | capi.STATUS_NONFINITE and s[1] == n_step
        assert not np.isfinite(q[1]).all()
        _check(capi, (q[fin], s[fin], t[fin], V[fin]), want, "edge fused=%s" % fused,
               peaks_ref.PeaksRef(D, B, fw), seeds[fin], f_lim)
        assert np.array_equal(q[7], seeds[7]) and t[7] == capi.PEAK_CONVERGED
        # the faint-at-once seed reports its initial V
        assert abs(V[8] - want["V"][7]) <= 1e-10 * abs(want["V"][7])
        # the NaN seed's wave-mates: as without it
        qm, sm, tm, Vm = _run(capi, D, B, fw, seeds[[0, 2, 3]], f_lim, n_step, fused=fused)
        assert np.array_equal(sm, s[[0, 2, 3]]) and np.array_equal(tm, t[[0, 2, 3]])


def _mock(side, fwhm, seed):
    """A small mock image and seeds for the configurations off the fused path."""
    from rhmc_amd.photometry import gauss_PSF, mag2flux, default_exp_setup
    _, _, f2c, _, B, _, mB, _ = default_exp_setup()
    rs = np.random.RandomState(seed)
    stars = [(19.5, 0.3 * side + 0.3, 0.6 * side + 0.4), (20.5, 0.7 * side + 0.2, 0.3 * side)]
    M = np.ones((side, side)) * B
    for m, x, y in stars:
        M += mag2flux(m) * f2c * gauss_PSF(side, side, x, y, FWHM=fwhm)
    D = rs.poisson(M).astype(np.float64)
    f_lim = mag2flux(mB - 1.) * f2c
    f_seed = mag2flux(mB - 1.5) * f2c
    seeds = [[f_seed, x + dx, y + dy] for _, x, y in stars for dx, dy in ((1.2, -0.8), (-2.5, 1.5))]
    seeds += [[f_seed, 0.5 * side, 0.9 * side], [f_seed, 0.1 * side, 0.1 * side],
              [f_seed, 0.9 * side, 0.8 * side]]
    return D, B, np.array(seeds), f_lim


@pytest.mark.parametrize("side,fwhm,kernel", [(40, 3.5, None), (32, 1.6 * 2.354, None),
                                               (32, 3.5, "generic")],
                         ids=["40px", "sigma1.6", "forced-generic"])
def test_configurations_off_the_fused_kernel(gpu_lib, side, fwhm, kernel):
    """A 40-px image, a 32-px image with sigma = 1.6 px (too wide for the 28-px
    window) and a forced per-wave family run the stepwise path on their own
    (RHMC_OPT_PEAKS_FUSED left at 1) and match peaks_ref."""
    capi = gpu_lib
    D, B, seeds, f_lim = _mock(side, fwhm, 11)
    n_step = 1000
    want = _want_ref(("off", side, fwhm), D, B, fwhm, seeds, f_lim, n_step)
    assert len(set(want["reasons"])) >= 2, want["reasons"]   # the seeds stop in more than one way
    got = _run(capi, D, B, fwhm, seeds, f_lim, n_step, kernel=kernel)
    _check(capi, got, want, "side %d fwhm %.3f %s" % (side, fwhm, kernel),
           peaks_ref.PeaksRef(D, B, fwhm), seeds, f_lim)


def test_device_entry_on_a_stream_and_empty_batch(gpu_lib):
    """rhmc_find_peaks_device on torch tensors on a non-default stream equals
    the host entry bit for bit; n = 0 returns 0."""
    import ctypes
    import torch
    capi = gpu_lib
    z = _golden()
    grid = z["A60/grid"]
    n = len(grid)
    q, s, t, V = _run_case(capi, "A60", True)
    ctx = capi.Context(z["A60/D"], device=0)
    P = _params(capi, float(z["A60/B_count"]), float(z["A60/fwhm_pix"]))
    opts = capi.make_peaks_opts(float(z["A60/f_lim"]), n_step=int(z["A60/Nstep"]))
    dev = torch.device("cuda:0")
    stream = torch.cuda.Stream()
    q_d = torch.from_numpy(grid.copy()).to(dev)
    s_d = torch.zeros(n, dtype=torch.int32, device=dev)
    t_d = torch.zeros(n, dtype=torch.int32, device=dev)
    V_d = torch.zeros(n, dtype=torch.float64, device=dev)
    torch.cuda.synchronize()
    ctx.find_peaks_device(P, opts, q_d.data_ptr(), n, s_d.data_ptr(), t_d.data_ptr(),
                          V_d.data_ptr(), stream.cuda_stream)
    stream.synchronize()
    assert np.array_equal(q_d.cpu().numpy(), q) and np.array_equal(V_d.cpu().numpy(), V)
    assert np.array_equal(s_d.cpu().numpy(), s) and np.array_equal(t_d.cpu().numpy(), t)
    # nullable outputs
    q2_d = torch.from_numpy(grid.copy()).to(dev)
    torch.cuda.synchronize()
    ctx.find_peaks_device(P, opts, q2_d.data_ptr(), n, None, None, None, stream.cuda_stream)
    stream.synchronize()
    assert np.array_equal(q2_d.cpu().numpy(), q)
    one = np.zeros(3)
    rc = capi.lib().rhmc_find_peaks(ctx.handle, ctypes.byref(P), ctypes.byref(opts),
                                    one.ctypes.data_as(ctypes.POINTER(ctypes.c_double)), 0,
                                    None, None, None)
    assert rc == 0
    ctx.close()


def test_pipeline_end_to_end(gpu_lib, capsys):
    """Case B: gym.find_peaks() gives the reference's merged q_seed, then
    HMC_find_best_dt(default=True) and HMC_random(q_model_0=None) run."""
    from rhmc_amd.samplers import lightsource_gym
    z = _golden()
    g = lightsource_gym()
    g.num_rows = g.num_cols = int(z["B/side"])
    np.random.seed(int(z["B/seed"]))
    g.gen_mock_data(z["B/q_true"])
    assert np.array_equal(g.D, z["B/D"])
    g.find_peaks(linear_pix_density=float(z["B/density"]), Nstep=int(z["B/Nstep"]))
    want = z["B/merge_out"]
    assert g.q_seed.shape == want.shape
    assert (np.abs(g.q_seed - want) / (np.abs(want) + 1)).max() <= 1e-9
    assert np.array_equal(g.peak_steps, z["B/steps"])
    g.HMC_find_best_dt(default=True)
    np.testing.assert_allclose(g.dt, z["B/dt_default"], rtol=1e-9)
    g.HMC_random(q_model_0=None, Niter=5)
    assert g.q_chain.shape == (1, 6, g.d) and np.isfinite(g.q_chain).all()
    assert np.array_equal(g.q_chain[0, 0], g.q_seed.reshape(-1))
