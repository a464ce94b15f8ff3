"""Every kernel body of the ragged implicit step.

rhmc_leapfrog_ragged_device (csrc/rhmc_launch.hpp: launch_leapfrog_ragged)
launches one of 13 kernel bodies: leapfrog_pk<32|48, 10, IMPLICIT, true>, the
RAGGED instantiations no fixed-K call reaches, and leapfrog_win_kernel<G, SLOTS>
with G = DenseG<32|48> in 1, 2, 4 slots, WinG in one and WinGG in 2, 4, 8, 16.
TABLE holds at least one ragged set per body with the body's key beside it;
tests/test_ragged_bodies.py checks on the CPU (tests/native/traj_bodies.cpp in
its `ragged` mode) that every set is served by the body written here at every
chain count launched below, that every star count of its [K_min, K_max] has the
set's ragged family and register slots, and that the table covers all 13.

A set is laid out as the reversible-jump driver lays its own out: rows of
ld = 3 K_max + 7 doubles, more rows than chains, launch chain j in row
order[j] of a permutation of a subset of the rows, d_K indexed by row.  Its
star counts hold the lowest of the slot class that shares the family, K_max,
one between and one twice; 5 chains leave the last workgroup of a slotted
kernel (four waves, one chain each) with one wave, and the pixel-major
kernel's last wave with one real chain and its mirror; launch chains 0 and 1,
one wave of the pixel-major kernel, are the lowest star count and K_max.

Every set runs:

* `free` against oracle.rhmc_ref.RefModel.step, each chain at its own K:
  every step from the oracle's previous state, uploaded into the rows before
  one ragged launch per step, at test_gpu_step_bodies.STEP_BAR (1e-11 q,
  1e-10 p of |value| + 1); all steps in one launch at FUSED_BAR (1e-9 / 1e-8).
* equal to fixed K: each chain's live columns equal rhmc_leapfrog on that
  chain alone, bit for bit (include/rhmc.h's promise).
* hostile padding: the same launch with zeros, then with quiet NaNs of a
  recognisable payload, in every column >= 3 K[row] of q and p and in every
  unused row, d_K of the unused rows 0, then 0 and K_max + 1 in turn.  The
  live columns of the two are bit-identical, and compared as uint64 every
  padding column and unused row is unchanged: the kernel reads nothing there
  and writes nothing there, not even zeros.
* rows = NULL on an unpermuted copy: bit-identical to the permuted run.
* a degenerate set, K_min == K_max: bit-identical to one fixed-K call.

One set per family (pixel-major, dense, WinG, WinGG) also runs `edge` (the
last star of the lowest-K chain, launch chain 0, leaves through x = 0 beside
the K_max chain) and `wall` (the same chain's last star goes below the flux
wall on a chosen step); the ragged call returns no status word, so the check is
q and p against the oracle at the fused bar.  `vc`: the pair potential on
(beta and Vc_r_pow of golden vc5) with star K - 1 of the K_max chain on star
1, in another slot where there are two; the pixel-major kernel does not serve
the pair potential (csrc/rhmc_select.hpp: use_pixk; tests/test_ragged_bodies.py
asserts that no ragged family is left there), so its set has no `vc`.  The
pixel-major sets, the one ragged body with two chains in a wave, also start a
chain with a NaN flux: the others, its wave-mate of another K among them, stay
within test_gpu_step_bodies.NAN_ROWS' pixel-major bar, 1e-12.

conditions() asserts on the CPU the conditions under which the bars hold,
test_gpu_step_bodies' own per chain (fixed-point test values outside
delta (1 +- 1e-9), nothing within 1e-7 relative of a wall, a 1 +- 1e-13 scaling
of dphidq moves the end state by at most a tenth of the bar).  No chain is
skipped and no set takes a looser bar.  DESIGN section 4j has the measured
figures per body.
"""
import numpy as np
import pytest

import test_gpu_step_bodies as G
from rhmc_amd.photometry import default_exp_setup, mag2flux
from test_gpu_energy_bodies import VC_BETA, VC_POW
from test_gpu_rhmc_diag import WALL_MAG, _rel_each
from test_gpu_step_bodies import FUSED_BAR, REF_FWHM, STEP_BAR, XY, F

pytestmark = pytest.mark.gpu

NAN_BAR = G.NAN_ROWS["k2_pixmajor32"]       # 1e-12
PAYLOAD = np.uint64(0x7FF8DEAD0000BEEF)     # a quiet NaN no arithmetic produces
SPARE_ROWS = 3                              # rows of the arrays no chain uses
N_DEGENERATE = 3


def _set(side, kernel, fwhm, body, Ks, f32=True):
    return (side, kernel, f32, fwhm, body, tuple(Ks))


# id: image side, forced kernel, image exact in fp32, PSF FWHM, body key, the
# star count of each launch chain (the first the lowest of the slot class that
# shares the family, the second K_max)
TABLE = {
    # pixel-major, 2-10 stars: chains 0 and 1 (2 and 10 stars) share a wave
    "pk32": _set(32, None, REF_FWHM, "pixmajor/32/ragged", [2, 10, 5, 10, 7]),
    "pk48": _set(48, None, REF_FWHM, "pixmajor/48/ragged", [2, 10, 3, 9, 3]),
    # dense by rule from 11 stars; forced, from one: a one-star chain beside a
    # ten-star chain
    "dense32_s1": _set(32, None, REF_FWHM, "slotted/Dense32/1", [11, 14, 12, 14, 13]),
    "dense32_forced": _set(32, "dense", REF_FWHM, "slotted/Dense32/1", [1, 10, 5, 10, 1]),
    "dense32_s2": _set(32, None, REF_FWHM, "slotted/Dense32/2", [65, 70, 67, 70, 65]),
    "dense32_s4": _set(32, None, REF_FWHM, "slotted/Dense32/4", [129, 256, 193, 256, 129]),
    "dense48_s1": _set(48, None, REF_FWHM, "slotted/Dense48/1", [11, 14, 12, 12, 11]),
    "dense48_s2": _set(48, None, REF_FWHM, "slotted/Dense48/2", [65, 70, 66, 70, 68]),
    "dense48_s4": _set(48, None, REF_FWHM, "slotted/Dense48/4", [129, 132, 130, 132, 131]),
    # LDS tables: by rule below the register kernels' 32 px (from 17 stars:
    # up to 16 the LDS-image kernel, a fixed K per launch), forced on 48 px
    "wing24": _set(24, None, REF_FWHM, "slotted/WinG/1", [17, 40, 28, 40, 17]),
    "wing48_forced": _set(48, "windowed", REF_FWHM, "slotted/WinG/1", [2, 64, 30, 64, 2]),
    # global tables
    "wingg64_s2": _set(64, None, REF_FWHM, "slotted/WinGG/2", [65, 70, 67, 70, 65]),
    "wingg64_s4": _set(64, None, REF_FWHM, "slotted/WinGG/4", [129, 132, 130, 132, 131]),
    "wingg32_s8": _set(32, None, REF_FWHM, "slotted/WinGG/8", [257, 260, 258, 260, 257]),
    "wingg32_s16": _set(32, None, REF_FWHM, "slotted/WinGG/16", [513, 520, 516, 520, 513]),
    "wingg32_k1024": _set(32, None, REF_FWHM, "slotted/WinGG/16", [513, 1024, 768, 1024, 513]),
}
# one set per family for edge, wall, vc (two slots where the family has them)
FAMILY_ROWS = {"pixmajor": "pk32", "dense": "dense32_s2", "WinG": "wing48_forced",
               "WinGG": "wingg64_s2"}
VC_ROWS = [FAMILY_ROWS[f] for f in ("dense", "WinG", "WinGG")]
NAN_ROWS = ["pk32", "pk48"]
_cache = {}


def Ks_of(name):
    return TABLE[name][5]


def shape(name, n=None):
    """The set as a row of test_gpu_step_bodies.TABLE at K_max: its field,
    parameters and step count are that file's."""
    side, kernel, f32, fwhm, body, Ks = TABLE[name]
    return (max(Ks), side, len(Ks) if n is None else n, kernel, 0, fwhm, f32, G._steps(max(Ks)),
            body)


def steps_of(name):
    return shape(name)[7]


def launch_counts(name):
    """Every chain count a ragged launch of the set has below."""
    return sorted({len(Ks_of(name)), N_DEGENERATE})


def scenarios(name):
    return ["free"] + (["edge", "wall"] if name in FAMILY_ROWS.values() else []) \
        + (["vc"] if name in VC_ROWS else [])


def layout(name, n=None):
    """(rows of the arrays, ld, order): launch chain j is row order[j]."""
    Ks = Ks_of(name)
    n = len(Ks) if n is None else n
    n_rows = n + SPARE_ROWS
    rng = np.random.RandomState(max(Ks) + n)
    order = rng.permutation(n_rows)[:n]
    while np.array_equal(order, np.sort(order)):    # never the rows in order
        order = rng.permutation(n_rows)[:n]
    return n_rows, 3 * max(Ks) + 7, order


# ------------------------------------------------------------- the CPU cases
def _start(name):
    """(D, q0, z): the field of test_gpu_step_bodies at K_max; chain c keeps
    its first Ks[c] stars."""
    Ks = Ks_of(name)
    D, q0, z = G._start(shape(name))
    return D, [q0[c, :3 * K].copy() for c, K in enumerate(Ks)], \
        [z[c, :3 * K].copy() for c, K in enumerate(Ks)]


def _momenta(name, D, par, q0, z):
    m = G._model(shape(name), D, par)
    return [zc * np.sqrt(m.H(q)) for q, zc in zip(q0, z)]


def _vc(par):
    return dict(par, use_Vc=True, beta=VC_BETA, Vc_r_pow=VC_POW)


def free_case(name):
    if ("free", name) not in _cache:
        D, q0, z = _start(name)
        par = G._par(shape(name), True, 0.)
        p0 = _momenta(name, D, par, q0, z)
        out = G._case(shape(name), "free", D, par, q0, p0, [steps_of(name)] * len(q0), FUSED_BAR,
                      stepwise=True)
        assert all(w["st"] == 0 for w in out["want"]), name
        _cache[("free", name)] = out
    return _cache[("free", name)]


def edge_case(name):
    """The last star of launch chain 0 (the lowest K) starts 0.3 px inside
    x = 0 and moves outwards half a pixel per step."""
    if ("edge", name) not in _cache:
        D, q0, z = _start(name)
        par = G._par(shape(name), True, 0.)
        p0 = _momenta(name, D, par, q0, z)
        m = G._model(shape(name), D, par)
        i = 3 * (Ks_of(name)[0] - 1) + 1
        q0[0][i] = 0.3
        p0[0][i] = -0.5 / par["dt"] * m.H(q0[0])[i]
        out = G._case(shape(name), "edge", D, par, q0, p0, [steps_of(name)] * len(q0), FUSED_BAR)
        st = [w["st"] for w in out["want"]]
        assert st[0] == XY and not any(st[1:]), (name, st)
        _cache[("edge", name)] = out
    return _cache[("edge", name)]


def wall_case(name):
    """No prior, the wall at WALL_MAG: the last star of launch chain 0 starts
    2 % above it with the momentum that takes it below on the latest of steps
    3, 2, 1 (2, 1 from 65 stars) it can be aimed at; every chain runs the set's
    steps, so chain 0 runs on past its flip beside the K_max chain."""
    if ("wall", name) not in _cache:
        D, q0, z = _start(name)
        steps = steps_of(name)
        f_lim = mag2flux(WALL_MAG) * default_exp_setup()[2]
        par = G._par(shape(name), False, f_lim)
        p0 = _momenta(name, D, par, q0, z)
        m = G._model(shape(name), D, par)
        i = 3 * (Ks_of(name)[0] - 1)
        q0[0][i] = f_lim * 1.02
        for t in ((3, 2, 1) if steps >= 8 else (2, 1)):
            if G._aim(m, par, q0[0], p0[0], i, t, steps, f_lim):
                break
        else:
            raise AssertionError((name, "no crossing step"))
        out = G._case(shape(name), "wall", D, par, q0, p0, [steps] * len(q0), FUSED_BAR)
        out.update(f_lim=f_lim, t=t)
        st = [w["st"] for w in out["want"]]
        assert st[0] & F and st[1] == 0, (name, st)
        _cache[("wall", name)] = out
    return _cache[("wall", name)]


def vc_case(name):
    """The pair potential on; in launch chain 1 (K_max stars) star K - 1 sits
    on star 1: the R < 1e-10 branch, across two slots where there are two."""
    if ("vc", name) not in _cache:
        D, q0, z = _start(name)
        Ks = Ks_of(name)
        par = _vc(G._par(shape(name), True, 0.))
        K = Ks[1]
        assert K == max(Ks) and (win_slots(K) == 1 or (K - 1) // 64 != 0)
        q0[1][3 * (K - 1) + 1: 3 * K] = q0[1][4:6]
        p0 = _momenta(name, D, par, q0, z)
        out = G._case(shape(name), "vc", D, par, q0, p0, [steps_of(name)] * len(q0), FUSED_BAR)
        _cache[("vc", name)] = out
    return _cache[("vc", name)]


def win_slots(K):
    """csrc/rhmc_select.hpp: star slots per lane of the slotted kernels."""
    return 1 if K <= 64 else 2 if K <= 128 else 4 if K <= 256 else 8 if K <= 512 else 16


CASES = {"free": free_case, "edge": edge_case, "wall": wall_case, "vc": vc_case}


def conditions(name):
    """Every scenario of a set on the CPU; {scenario: (conditioning as a
    fraction of the bar, least delta margin, least wall clearance)}."""
    out = {}
    for scen in scenarios(name):
        c = CASES[scen](name)
        out[scen] = (c["cond"], c["margin"], c["clear"])
    return out


# ------------------------------------------------------------------- the GPU
class _Ctx(G._Ctx):
    def __init__(self, capi, name, case):
        self.ctx = capi.Context(case["D"], kernel=TABLE[name][1] or "auto")


def live_mask(n_rows, ld, order, Ks):
    live = np.zeros((n_rows, ld), bool)
    for j, r in enumerate(order):
        live[r, :3 * Ks[j]] = True
    return live


class Rows:
    """A ragged set on the device in the driver's layout.  hostile: the
    padding columns, the unused rows and the unused rows' d_K are poison."""

    def __init__(self, qs, ps, n_rows, ld, order, hostile=False):
        import torch
        self.Ks = [len(q) // 3 for q in qs]
        self.n_rows, self.ld, self.order = n_rows, ld, None if order is None else np.asarray(order)
        rows = np.arange(len(qs)) if order is None else self.order
        fill = PAYLOAD if hostile else np.uint64(0)
        self.q0 = np.full((n_rows, ld), fill, np.uint64).view(np.float64)
        self.p0 = self.q0.copy()
        K_of = np.zeros(n_rows, np.int32)
        unused = sorted(set(range(n_rows)) - set(rows.tolist()))
        if hostile:     # 0 would fault or corrupt if read, K_max + 1 computes on the poison
            K_of[unused[1::2]] = max(self.Ks) + 1
        for j, r in enumerate(rows):
            self.q0[r, :3 * self.Ks[j]] = qs[j]
            self.p0[r, :3 * self.Ks[j]] = ps[j]
            K_of[r] = self.Ks[j]
        self.rows = rows
        self.live = live_mask(n_rows, ld, rows, self.Ks)
        assert 3 * (int(K_of.max())) <= ld and rows.max() < n_rows and len(set(rows)) == len(rows)
        dev = torch.device("cuda:0")
        self.qd = torch.from_numpy(self.q0.copy()).to(dev)
        self.pd = torch.from_numpy(self.p0.copy()).to(dev)
        self.Kd = torch.from_numpy(K_of).to(dev)
        self.rd = None if order is None else torch.from_numpy(rows.astype(np.int64)).to(dev)

    def step(self, ctx, P, n_steps):
        """One ragged launch; the chains' (q, p) lists, and the whole arrays."""
        import torch
        ctx.leapfrog_ragged_device(P, self.qd.data_ptr(), self.pd.data_ptr(), self.ld,
                                   0 if self.rd is None else self.rd.data_ptr(),
                                   self.Kd.data_ptr(), len(self.Ks), min(self.Ks), max(self.Ks),
                                   n_steps)
        torch.cuda.synchronize()
        self.q, self.p = self.qd.cpu().numpy(), self.pd.cpu().numpy()
        return ([self.q[r, :3 * K] for r, K in zip(self.rows, self.Ks)],
                [self.p[r, :3 * K] for r, K in zip(self.rows, self.Ks)])

    def untouched(self):
        """Compared as uint64, everything but the live columns is as uploaded."""
        dead = ~self.live
        return all(np.array_equal(a.view(np.uint64)[dead], b.view(np.uint64)[dead])
                   for a, b in ((self.q, self.q0), (self.p, self.p0)))


def _rows(name, qs, ps, hostile=False, permuted=True):
    n_rows, ld, order = layout(name, len(qs))
    return Rows(qs, ps, n_rows, ld, order if permuted else None, hostile)


def _errors(q, p, want_q, want_p):
    return (max(_rel_each(a, b) for a, b in zip(q, want_q)),
            max(_rel_each(a, b) for a, b in zip(p, want_p)))


def _same(a, b):
    return all(np.array_equal(x, y) for x, y in zip(a, b))


def _report(capsys, name, run, case, text):
    with capsys.disabled():
        print("\n  %s %s [%s]: %s; conditioning %.2g of the bar, delta margin %.2g, CPU %.1f s"
              % (name, run, TABLE[name][4], text, case["cond"], case["margin"], case["cpu_s"]))


def _fused(capi, ctx, name, case, hostile=False):
    """All steps in one ragged launch against the oracle: (eq, ep)."""
    P = capi.make_params(**case["par"])
    r = _rows(name, case["q0"], case["p0"], hostile)
    q, p = r.step(ctx, P, steps_of(name))
    assert r.untouched()
    return _errors(q, p, [w["Q"][-1] for w in case["want"]], [w["P"][-1] for w in case["want"]])


@pytest.mark.parametrize("name", list(TABLE))
def test_free_stepwise_and_fused(gpu_lib, name, capsys):
    capi = gpu_lib
    case = free_case(name)
    want, steps = case["want"], steps_of(name)
    P = capi.make_params(**case["par"])
    sq = sp = 0.
    with _Ctx(capi, name, case) as ctx:
        for k in sorted(set(Ks_of(name))):
            assert ctx.ragged_ok(P, k), k
        for s in range(steps):      # each step from the oracle's own state
            r = _rows(name, [w["Q"][s] for w in want], [w["P"][s] for w in want])
            q, p = r.step(ctx, P, 1)
            eq, ep = _errors(q, p, [w["Q"][s + 1] for w in want], [w["P"][s + 1] for w in want])
            sq, sp = max(sq, eq), max(sp, ep)
        fq, fp = _fused(capi, ctx, name, case)
    _report(capsys, name, "free", case, "stepwise q %.2g p %.2g of the bars (%.2g, %.2g), fused "
            "q %.2g p %.2g of the bars (%.2g, %.2g)"
            % (sq / STEP_BAR[0], sp / STEP_BAR[1], sq, sp, fq / FUSED_BAR[0], fp / FUSED_BAR[1],
               fq, fp))
    assert sq <= STEP_BAR[0] and sp <= STEP_BAR[1]
    assert fq <= FUSED_BAR[0] and fp <= FUSED_BAR[1]


@pytest.mark.parametrize("name", list(TABLE))
def test_equal_to_fixed_K(gpu_lib, name):
    """Each chain's live columns equal rhmc_leapfrog on that chain alone."""
    capi = gpu_lib
    case = free_case(name)
    P = capi.make_params(**case["par"])
    with _Ctx(capi, name, case) as ctx:
        q, p = _rows(name, case["q0"], case["p0"]).step(ctx, P, steps_of(name))
        for c, (q0, p0) in enumerate(zip(case["q0"], case["p0"])):
            q1, p1 = ctx.leapfrog(P, q0[None], p0[None], steps_of(name))
            assert np.array_equal(q[c], q1[0]) and np.array_equal(p[c], p1[0]), (c, len(q0) // 3)


@pytest.mark.parametrize("name", list(TABLE))
def test_hostile_padding(gpu_lib, name):
    """Zeros, then NaNs of a known payload, past 3 K[row] and in the unused
    rows, and d_K of the unused rows 0, then 0 / K_max + 1: the live columns
    bit-identical, everything else untouched as uint64."""
    capi = gpu_lib
    case = free_case(name)
    P = capi.make_params(**case["par"])
    with _Ctx(capi, name, case) as ctx:
        clean = _rows(name, case["q0"], case["p0"])
        q, p = clean.step(ctx, P, steps_of(name))
        hostile = _rows(name, case["q0"], case["p0"], hostile=True)
        assert hostile.Kd.cpu().numpy().max() == max(Ks_of(name)) + 1
        assert np.isnan(hostile.q0[~hostile.live]).all() and (~hostile.live).sum() > hostile.ld
        qh, ph = hostile.step(ctx, P, steps_of(name))
    assert np.isfinite(np.concatenate(q + p)).all()
    assert _same(qh, q) and _same(ph, p)
    assert clean.untouched() and hostile.untouched()


@pytest.mark.parametrize("name", list(TABLE))
def test_rows_null(gpu_lib, name):
    """rows = NULL: chain j in row j of an unpermuted copy."""
    capi = gpu_lib
    case = free_case(name)
    P = capi.make_params(**case["par"])
    with _Ctx(capi, name, case) as ctx:
        q, p = _rows(name, case["q0"], case["p0"]).step(ctx, P, steps_of(name))
        ident = _rows(name, case["q0"], case["p0"], hostile=True, permuted=False)
        qi, pi = ident.step(ctx, P, steps_of(name))
    assert _same(qi, q) and _same(pi, p) and ident.untouched()


@pytest.mark.parametrize("name", list(TABLE))
def test_degenerate_set(gpu_lib, name):
    """K_min == K_max: the fixed-K call on the same chains."""
    capi = gpu_lib
    case = free_case(name)
    K, steps = max(Ks_of(name)), steps_of(name)
    D, q0, z = G._start(shape(name))
    q0, z = q0[:N_DEGENERATE], z[:N_DEGENERATE]
    m = G._model(shape(name), D, case["par"])
    p0 = z * np.sqrt(np.array([m.H(q) for q in q0]))
    P = capi.make_params(**case["par"])
    with _Ctx(capi, name, case) as ctx:
        r = _rows(name, list(q0), list(p0), hostile=True)
        assert r.Ks == [K] * N_DEGENERATE
        q, p = r.step(ctx, P, steps)
        q1, p1 = ctx.leapfrog(P, q0, p0, steps)
    assert np.array_equal(np.array(q), q1) and np.array_equal(np.array(p), p1) and r.untouched()
    assert np.isfinite(q1).all() and np.isfinite(p1).all()


@pytest.mark.parametrize("name,scen", [(name, scen) for name in FAMILY_ROWS.values()
                                       for scen in scenarios(name)[1:]])
def test_family_scenarios(gpu_lib, name, scen, capsys):
    """edge, wall, vc on one set per family, under hostile padding."""
    capi = gpu_lib
    case = CASES[scen](name)
    with _Ctx(capi, name, case) as ctx:
        eq, ep = _fused(capi, ctx, name, case, hostile=True)
    _report(capsys, name, scen, case, "q %.2g p %.2g of the bars (%.2g, %.2g)"
            % (eq / FUSED_BAR[0], ep / FUSED_BAR[1], eq, ep))
    assert eq <= FUSED_BAR[0] and ep <= FUSED_BAR[1]


@pytest.mark.parametrize("name", NAN_ROWS)
def test_nan_chain_beside_a_wave_mate_of_another_K(gpu_lib, name):
    """Launch chain 1 (K_max stars) starts with a NaN flux: its wave-mate, chain
    0 with the lowest K, and the other chains as without it."""
    capi = gpu_lib
    case = free_case(name)
    P = capi.make_params(**case["par"])
    qb = [q.copy() for q in case["q0"]]
    qb[1][0] = np.nan
    assert Ks_of(name)[0] != Ks_of(name)[1]
    with _Ctx(capi, name, case) as ctx:
        q, p = _rows(name, case["q0"], case["p0"]).step(ctx, P, steps_of(name))
        bad = _rows(name, qb, case["p0"], hostile=True)
        q2, p2 = bad.step(ctx, P, steps_of(name))
    assert np.isnan(q2[1][0]) and bad.untouched()
    others = [c for c in range(len(qb)) if c != 1]
    eq, ep = _errors([q2[c] for c in others], [p2[c] for c in others],
                     [q[c] for c in others], [p[c] for c in others])
    assert eq <= NAN_BAR and ep <= NAN_BAR, (eq, ep)
