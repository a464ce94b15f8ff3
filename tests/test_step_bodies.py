"""Which kernel body serves the implicit generalized-leapfrog step, on the CPU.

tests/native/traj_bodies.cpp in its `step` mode (a host compiler,
csrc/rhmc_select.hpp and csrc/rhmc_dispatch.hpp alone) names the body that
rhmc_leapfrog launches for a shape, by calling the switches of
rhmc_dispatch.hpp that csrc/rhmc_launch.hpp's launchers call (launch_leapfrog:
launch_tiledr, launch_tiledl, launch_multi, launch_kr, launch_leap_slotted;
the LDS-image step in launch_leapfrog itself).  Unlike the other two
operations the step's body depends on
the chain count, on RHMC_OPT_WINDOW_SPLIT and on the PSF width, so the program
takes those per case.  BODIES is written from the instantiations those
switches can reach, not from the program:

* the sweep (sides 32/40/48/64/96/128/256, K = 1..1024, fp32-exact or not,
  every RHMC_KERNEL_* value, 4 / 16384 / 65536 chains, window split 0/1/2/4,
  the reference PSF and FWHM 3.8 px) yields exactly these 64, and an
  unsupported plan only where the PSF is too wide for the 32-px windows of the
  slotted kernels (the program leaves exactly those out),
* every row of tests/test_gpu_step_bodies.py's TABLE runs the body written
  beside it at every chain count its tests launch, and the table covers all 64,
* every row's scenarios pass their conditioning assertions on the oracle.

A new body, or a moved threshold, fails here until a GPU row covers it."""
import pytest

import test_gpu_step_bodies as G
from rhmc_amd import capi
from test_gpu_step_bodies import TABLE
from test_traj_bodies import traj_bodies  # noqa: F401 (the fixture)

_DT = ("float", "double")
BODIES = sorted(
    # leapfrog_k1_tiledr<IMG, WIN, DT>
    ["regwin1/%d/%d/%s" % (img, win, dt) for img in (32, 48, 64, 96, 128) for win in (28, 32)
     for dt in _DT]
    # leapfrog_k1_tiledl<IMG, 28, DT, LPC>
    + ["lane/%d/%s/%d" % (img, dt, lpc) for img in (32, 48, 64) for dt in _DT for lpc in (1, 4)]
    # leapfrog_pk<IMG, 10, IMPLICIT>
    + ["pixmajor/32", "pixmajor/48"]
    # leapfrog_kr<DT, 1, true, IMPLICIT, 1>
    + ["multiwin/%s/1/tab" % dt for dt in _DT]
    # leapfrog_kr<DT, SLOTS, false, IMPLICIT, WS>
    + ["multiwin/%s/%d/notab/%d" % (dt, slots, ws) for dt in _DT for slots in (1, 2)
       for ws in (1, 2, 4)]
    # leapfrog_kernel<MAXK>
    + ["ldsimage/%d" % k for k in (1, 2, 4, 8, 16)]
    # leapfrog_win_kernel<G, SLOTS>
    + ["slotted/WinG/1"] + ["slotted/WinGG/%d" % s for s in (2, 4, 8, 16)]
    + ["slotted/Dense%d/%d" % (img, s) for img in (32, 48) for s in (1, 2, 4)])


def test_the_sweep_yields_the_64_bodies(traj_bodies):
    assert len(BODIES) == 64 == len(set(BODIES))
    keys = traj_bodies("step", "sweep")
    assert "Unsupported" not in keys
    assert sorted(keys) == BODIES


def _args(name, n):
    K, side, _, kernel, split, fwhm, f32, _, _ = TABLE[name]
    return [side, K, int(f32), capi.KERNELS[kernel or "auto"], n, split, fwhm]


def test_every_gpu_row_runs_the_body_written_beside_it(traj_bodies):
    """At every chain count the GPU tests launch for the row: all chains, the
    batch-invariance subset, the one-chain rerun, the wall's even and odd chains."""
    rows, args = [], []
    for name, row in TABLE.items():
        assert row[2] >= 2 and row[7] >= 1
        for n in G.launch_counts(name):
            rows.append((name, n))
            args += _args(name, n)
    got = traj_bodies("step", *args)
    assert len(got) == len(rows)
    assert dict(zip(rows, got)) == {(name, n): TABLE[name][8] for name, n in rows}


def test_the_gpu_rows_cover_every_body():
    assert sorted({row[8] for row in TABLE.values()}) == BODIES
    assert set(G.CAP_ROWS) <= set(TABLE) and set(G.NAN_ROWS) <= set(TABLE)
    # the wave-sharing families each have a NaN row, every family a cap row
    assert {TABLE[n][8].split("/")[0] for n in G.NAN_ROWS} == {"regwin1", "lane", "pixmajor",
                                                               "multiwin"}
    assert {TABLE[n][8].split("/")[0] for n in G.CAP_ROWS} == {b.split("/")[0] for b in BODIES}


@pytest.mark.parametrize("name", list(TABLE))
def test_the_row_is_conditioned(name, capsys):
    """The conditions under which the GPU bars hold, on the oracle alone
    (test_gpu_step_bodies.conditions asserts them)."""
    figures = G.conditions(name)
    with capsys.disabled():
        print("\n  %s: %s" % (name, ", ".join(
            "%s %.2g of the bar (delta margin %.2g, wall clearance %.2g)" % ((k,) + v)
            for k, v in figures.items())))
