"""Which kernel body serves rhmc_energy, rhmc_gradient and rhmc_mh, on the CPU.

tests/native/traj_bodies.cpp in its `energy`, `gradient` and `mh` modes (a
host compiler, csrc/rhmc_select.hpp and csrc/rhmc_dispatch.hpp alone) names the
body that each operation launches for a shape, by calling the switches of
rhmc_dispatch.hpp that csrc/rhmc_launch.hpp's launchers call
(launch_energy, launch_energy_slotted; launch_gradient; run_mh, launch_mh_k1,
launch_mh_pk).  The pair potential
changes the energy's body, so the program takes use_Vc per case; rhmc_mh takes
RHMC_OPT_MH_FUSED in its place.  BODIES is written from the instantiations
those switches can reach, not from the program:

* the sweeps (sides 32/40/48/64/96/256, K = 1..1024, fp32-exact or not, every
  RHMC_KERNEL_* value, 4 and 65536 chains, use_Vc or RHMC_OPT_MH_FUSED 0/1,
  the reference PSF and FWHM 3.8 px) yield exactly these 22 / 16 / 8 + 2, and
  an unsupported plan only where the PSF is too wide for the 32-px windows of
  the slotted kernels (the program leaves exactly those out),
* every row of tests/test_gpu_energy_bodies.py's tables runs the body written
  beside it at every chain count its tests launch (and with the pair potential
  on where its `vc` scenario turns it on, and under RHMC_OPT_MH_FUSED = 0
  where the MH test reruns the loop), and the tables cover every body,
* every row passes its conditioning assertions on the oracle.

A new body, or a moved threshold, fails here until a GPU row covers it."""
import pytest

import test_gpu_energy_bodies as G
from rhmc_amd import capi
from test_traj_bodies import traj_bodies  # noqa: F401 (the fixture)

_DT = ("float", "double")
_PER_WAVE = (
    # energy_ / gradient_win_kernel<LdsG<MAXK>, 1>
    ["ldsimage/%d" % k for k in (1, 2, 4, 8, 16)]
    # energy_ / gradient_win_kernel<WinGG, SLOTS>, <DenseG<IMG>, SLOTS>
    + ["slotted/WinGG/%d" % s for s in (2, 4, 8, 16)]
    + ["slotted/Dense%d/%d" % (img, s) for img in (32, 48) for s in (1, 2, 4)])
BODIES = {
    # energy_k1_tiledr<IMG, DT>, energy_win_kernel<WinEG, 1>
    "energy": sorted(["regwin1/%d/%s" % (img, dt) for img in (32, 48, 64) for dt in _DT]
                     + ["slotted/WinEG/1"] + _PER_WAVE),
    # gradient_win_kernel<WinG, 1>
    "gradient": sorted(["slotted/WinG/1"] + _PER_WAVE),
    # mh_k1_tiledr<IMG, 28, DT>; mh_pk_v0 / mh_pk_iter<IMG, 10>; the loop's
    # mh_begin / mh_end kernels in their thread and wave forms
    "mh": sorted(["mh/regwin1/%d/%s" % (img, dt) for img in (32, 48, 64) for dt in _DT]
                 + ["mh/pixmajor/32", "mh/pixmajor/48"] + ["mh/loop/thread", "mh/loop/wave"]),
}
TABLES = {"energy": G.TABLE_E, "gradient": G.TABLE_G, "mh": G.TABLE_MH}
COUNTS = {"energy": 22, "gradient": 16, "mh": 8 + 2}


@pytest.mark.parametrize("op", list(BODIES))
def test_the_sweep_yields_the_bodies(traj_bodies, op):
    assert len(BODIES[op]) == COUNTS[op] == len(set(BODIES[op]))
    keys = traj_bodies(op, "sweep")
    assert "Unsupported" not in keys
    assert sorted(keys) == BODIES[op]


def _args(row, n, flag):
    K, side, _, kernel, _, fwhm, f32 = row[:7]
    return [side, K, int(f32), capi.KERNELS[kernel or "auto"], n, int(flag), fwhm]


@pytest.mark.parametrize("op", list(BODIES))
def test_every_gpu_row_runs_the_body_written_beside_it(traj_bodies, op):
    """At every chain count the GPU tests launch for the row (all chains, the
    subset, one chain; the energy's support and ragged sets), with the pair
    potential as the row has it and on where the `vc` scenario turns it on; an
    MH row under RHMC_OPT_MH_FUSED = 1 and, where the test reruns the loop, 0."""
    cases, args = {}, []
    for name, row in TABLES[op].items():
        assert 2 <= row[2] <= 5 or "regwin1" in row[7]
        flags = {row[4]: row[7]}
        if op == "mh" and row[8]:
            flags[0] = row[8]
        elif op != "mh" and name in G.VC_ROWS:
            flags[True] = row[7]
        for flag, body in flags.items():
            for n in G.launch_counts(op, name):
                cases[(name, n, int(flag))] = body
                args += _args(row, n, flag)
    got = traj_bodies(op, *args)
    assert len(got) == len(cases)
    assert dict(zip(cases, got)) == cases


def test_the_gpu_rows_cover_every_body():
    for op, table in TABLES.items():
        assert sorted({row[7] for row in table.values()}) == BODIES[op], op
    # the loop's two forms are also what the fused rows fall back to
    assert {row[8] for row in G.TABLE_MH.values() if row[8]} == {"mh/loop/thread", "mh/loop/wave"}
    assert {G.TABLE_MH[n][8] is None for n in G.TABLE_MH if "loop" in G.TABLE_MH[n][7]} == {True}
    E = G.TABLE_E
    # regwin1 rows: fp32-exact and not on every side, 17 chains once; a NaN row each
    assert {E[n][7] for n in G.NAN_ROWS} == {b for b in BODIES["energy"] if "regwin1" in b}
    assert sorted(E[n][2] for n in G.NAN_ROWS) == [5] * 5 + [17]
    # the pair potential in every other body, the coincident pair in two slots
    assert {E[n][7] for n in G.VC_ROWS} == {b for b in BODIES["energy"] if "regwin1" not in b}
    # a ragged set in every body one can reach (rhmc_select.hpp: ragged_family)
    assert {E[n][7] for n in G.RAGGED_ROWS} == \
        {b for b in BODIES["energy"] if "regwin1" not in b and b != "ldsimage/1"}
    for n, lo in G.RAGGED_ROWS.items():
        K = E[n][0]
        assert lo <= K and [a for a in (1, 65, 129, 257, 513) if a <= lo][-1] == \
            [a for a in (1, 65, 129, 257, 513) if a <= K][-1]
    # the MH loop at both sides of the K >= 8 switch and past 64 coordinates
    assert sorted(r[0] for r in G.TABLE_MH.values() if r[8] is None) == [3, 7, 8, 12, 70]


@pytest.mark.parametrize("name", list(G.TABLE_E))
def test_the_energy_row_is_conditioned(name, capsys):
    """test_gpu_energy_bodies.conditions_e asserts the conditions."""
    figures = G.conditions_e(name)
    with capsys.disabled():
        print("\n  energy %s: %s" % (name, ", ".join(
            "%s V %.2g T %.2g of the bar (clearance %.2g)" % ((k,) + v)
            for k, v in figures.items())))


@pytest.mark.parametrize("name", list(G.TABLE_G))
def test_the_gradient_row_is_conditioned(name, capsys):
    figures = G.conditions_g(name)
    with capsys.disabled():
        print("\n  gradient %s: %s" % (name, ", ".join("%s %.2g of the bar" % kv
                                                       for kv in figures.items())))


@pytest.mark.parametrize("name", list(G.TABLE_MH))
def test_the_mh_row_is_conditioned(name, capsys):
    margin, accepted = G.conditions_mh(name)
    with capsys.disabled():
        print("\n  mh %s: least |log u + dE| %.2g, accepted %.2f" % (name, margin, accepted))
