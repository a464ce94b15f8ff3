"""Which kernel bodies serve a ragged chain set, on the CPU.

tests/native/traj_bodies.cpp in its `ragged` mode (a host compiler,
csrc/rhmc_select.hpp and csrc/rhmc_dispatch.hpp alone) names, for a launch's
K_max, the body rhmc_leapfrog_ragged_device launches and the one
rhmc_energy_ragged_device does, by the switches their launchers call
(csrc/rhmc_launch.hpp: launch_leapfrog_ragged takes with_side2 for a
pixel-major plan, the RAGGED instantiation, else launch_leap_slotted's
with_policy; launch_energy_ragged takes launch_energy_slotted's
with_perwave_energy_policy), or `none` where ragged_family() is 0.  BODIES and
ENERGY_BODIES are written from the instantiations those switches can reach,
not from the program:

* the sweep (sides 24/32/40/48/64/96/256, K = 1..1024, fp32-exact or not,
  every RHMC_KERNEL_* value, 4 / 65536 chains, the pair potential off and on,
  the reference PSF and FWHM 3.8 px) yields exactly these 13 step bodies, 15
  energy bodies and 19 pairs, and never an unsupported plan,
* every set of tests/test_gpu_ragged_bodies.py's TABLE runs the body written
  beside it for its K_max at every chain count its tests launch, with the pair
  potential where `vc` turns it on; every star count of its [K_min, K_max] has
  the same body, hence the same non-zero ragged_family, and the same
  win_slots (what ragged_check demands); its lowest star count is the lowest
  of the slot class that shares the family; the table covers all 13,
* every set's scenarios pass their conditioning assertions on the oracle.

A new body, or a moved threshold, fails here until a GPU set covers it."""
import pytest

import test_gpu_ragged_bodies as R
from rhmc_amd import capi
from test_gpu_ragged_bodies import TABLE
from test_traj_bodies import traj_bodies  # noqa: F401 (the fixture)

BODIES = sorted(
    # leapfrog_pk<IMG, 10, IMPLICIT, true>
    ["pixmajor/32/ragged", "pixmajor/48/ragged"]
    # leapfrog_win_kernel<G, SLOTS>
    + ["slotted/WinG/1"] + ["slotted/WinGG/%d" % s for s in (2, 4, 8, 16)]
    + ["slotted/Dense%d/%d" % (img, s) for img in (32, 48) for s in (1, 2, 4)])
ENERGY_BODIES = sorted(
    # energy_win_kernel<LdsG<MAXK>, 1>: the pixel-major step's energy, 2-10 stars
    ["ldsimage/%d" % k for k in (2, 4, 8, 16)]
    # energy_win_kernel<G, SLOTS>
    + ["slotted/WinEG/1"] + ["slotted/WinGG/%d" % s for s in (2, 4, 8, 16)]
    + ["slotted/Dense%d/%d" % (img, s) for img in (32, 48) for s in (1, 2, 4)])
# the step and the energy of one K: the same policy and slots, but the
# pixel-major step with each LDS-image energy and WinG with WinEG
PAIRS = sorted(
    ["pixmajor/%d/ragged|ldsimage/%d" % (img, k) for img in (32, 48) for k in (2, 4, 8, 16)]
    + ["slotted/WinG/1|slotted/WinEG/1"]
    + ["%s|%s" % (b, b) for b in BODIES if b.startswith(("slotted/WinGG", "slotted/Dense"))])


def test_the_sweep_yields_the_13_step_bodies_15_energy_bodies_and_19_pairs(traj_bodies):
    assert len(BODIES) == 13 == len(set(BODIES))
    assert len(ENERGY_BODIES) == 15 == len(set(ENERGY_BODIES))
    assert len(PAIRS) == 19 == len(set(PAIRS))
    pairs = traj_bodies("ragged", "sweep")
    assert not [p for p in pairs if "Unsupported" in p or "no-" in p or "none" in p]
    assert sorted(pairs) == PAIRS
    assert sorted({p.split("|")[0] for p in pairs}) == BODIES
    assert sorted({p.split("|")[1] for p in pairs}) == ENERGY_BODIES


def _args(name, K, n, use_Vc=False):
    side, kernel, f32, fwhm, _, _ = TABLE[name]
    return [side, K, int(f32), capi.KERNELS[kernel or "auto"], n, int(use_Vc), fwhm]


def _step_keys(traj_bodies, points):
    got = traj_bodies("ragged", *[a for p in points for a in p])
    assert len(got) == len(points)
    return [g.split("|")[0] for g in got]


def test_every_gpu_set_runs_the_body_written_beside_it(traj_bodies):
    """For its K_max at every chain count the GPU tests launch, and under the
    pair potential where `vc` runs."""
    rows, points = [], []
    for name in TABLE:
        Ks = R.Ks_of(name)
        assert len(Ks) == 5 and R.steps_of(name) >= 1
        for n in R.launch_counts(name):
            for vc in sorted({"vc" in R.scenarios(name), False}):
                rows.append((name, n, vc))
                points.append(_args(name, max(Ks), n, vc))
    got = _step_keys(traj_bodies, points)
    assert dict(zip(rows, got)) == {r: TABLE[r[0]][4] for r in rows}


def test_every_star_count_of_a_set_has_its_family_and_slots(traj_bodies):
    """ragged_check's two demands on [K_min, K_max], and Ks' four members: the
    lowest star count of the slot class that shares the family, K_max, one
    between them and one twice."""
    for name in TABLE:
        Ks, body = R.Ks_of(name), TABLE[name][4]
        lo, hi = min(Ks), max(Ks)
        assert Ks[0] == lo and Ks[1] == hi and any(lo < K < hi for K in Ks)
        assert len(set(Ks)) < len(Ks)
        for vc in sorted({"vc" in R.scenarios(name), False}):
            keys = _step_keys(traj_bodies, [_args(name, K, len(Ks), vc) for K in range(lo, hi + 1)])
            assert set(keys) == {body}, (name, vc)      # one body: one family, one SLOTS
        assert {R.win_slots(K) for K in range(lo, hi + 1)} == {R.win_slots(hi)}
        below = _step_keys(traj_bodies, [_args(name, max(lo - 1, 1), len(Ks))])[0] if lo > 1 \
            else "none"
        assert below != body or R.win_slots(lo - 1) != R.win_slots(lo), (name, below)


def test_the_gpu_sets_cover_every_body(traj_bodies):
    assert sorted({row[4] for row in TABLE.values()}) == BODIES
    family = {"pixmajor": "pixmajor", "dense": "slotted/Dense", "WinG": "slotted/WinG/",
              "WinGG": "slotted/WinGG/"}
    assert set(R.FAMILY_ROWS) == set(family)
    for f, name in R.FAMILY_ROWS.items():
        assert TABLE[name][4].startswith(family[f])
    # the pair potential takes the pixel-major family's star counts off the
    # ragged sets, so its set has no `vc`; the others keep their body (above)
    pk = R.FAMILY_ROWS["pixmajor"]
    assert "vc" not in R.scenarios(pk)
    Ks = R.Ks_of(pk)
    got = traj_bodies("ragged", *[a for K in range(min(Ks), max(Ks) + 1)
                                  for a in _args(pk, K, len(Ks), True)])
    assert set(got) == {"none"}
    assert sorted(R.NAN_ROWS) == [n for n in TABLE if TABLE[n][4].startswith("pixmajor")]
    # two slots under `vc` where the family has them
    assert all(R.win_slots(max(R.Ks_of(R.FAMILY_ROWS[f]))) == 2 for f in ("dense", "WinGG"))


@pytest.mark.parametrize("name", list(TABLE))
def test_the_set_is_conditioned(name, capsys):
    """The conditions under which the GPU bars hold, on the oracle alone
    (test_gpu_step_bodies' own, asserted per chain at the chain's K)."""
    figures = R.conditions(name)
    with capsys.disabled():
        print("\n  %s: %s" % (name, ", ".join(
            "%s %.2g of the bar (delta margin %.2g, wall clearance %.2g)" % ((k,) + v)
            for k, v in figures.items())))
