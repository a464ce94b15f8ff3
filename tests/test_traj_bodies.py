"""Which kernel body serves a random-length trajectory, on the CPU.

tests/native/traj_bodies.cpp (a host compiler, csrc/rhmc_select.hpp and
csrc/rhmc_dispatch.hpp alone) names the body that rhmc_hmc_random /
rhmc_diag_random launch for a shape: it calls the switches of rhmc_dispatch.hpp
that csrc/rhmc_launch.hpp's launchers call, with functors that name the
template arguments.  BODIES is written from the instantiations those switches
can reach, not from the program:

* the sweep (sides 32/48/64/96, K = 1..1024, fp32-exact or not, every
  RHMC_KERNEL_* value, 4 and 65536 chains) yields exactly these 25 and never
  an unsupported plan,
* every case of tests/test_gpu_traj_bodies.py's TABLE runs the body written
  beside it, and the table covers all 25.

A new body, or a moved threshold, fails here until a GPU case covers it."""
import os
import shutil
import subprocess

import pytest

from conftest import PKG_DIR, ROOT
from rhmc_amd import capi
from test_gpu_traj_bodies import TABLE

BODIES = sorted(
    # (diag_)hmc_random_k1_tiledr<IMG, DT>
    ["regwin1/%d/%s" % (img, dt) for img in (32, 48, 64) for dt in ("float", "double")]
    # leapfrog_pk<IMG, 10, SOLVER>
    + ["pixmajor/32", "pixmajor/48"]
    # leapfrog_kr<DT, SLOTS, TAB, SOLVER, 1>
    + ["multiwin/%s/%s" % (dt, v) for dt in ("float", "double")
       for v in ("1/tab", "1/notab", "2/notab")]
    # (diag_)hmc_random_win_kernel<G, SLOTS>
    + ["slotted/WinG/1"] + ["slotted/WinGG/%d" % s for s in (2, 4, 8, 16)]
    + ["slotted/Dense%d/%d" % (img, s) for img in (32, 48) for s in (1, 2, 4)])


@pytest.fixture(scope="module")
def traj_bodies(tmp_path_factory):
    gxx = shutil.which("g++")
    if not gxx:
        pytest.skip("g++ not available")
    exe = str(tmp_path_factory.mktemp("traj_bodies") / "traj_bodies")
    subprocess.run([gxx, "-std=c++17", "-O1", "-Wall", "-Werror", "-I",
                    os.path.join(ROOT, "include"), "-I", os.path.join(PKG_DIR, "csrc"), "-o", exe,
                    os.path.join(ROOT, "tests", "native", "traj_bodies.cpp")], check=True)

    def run(*args):
        r = subprocess.run([exe] + [str(a) for a in args], capture_output=True, text=True,
                           timeout=120)
        assert r.returncode == 0, r.stdout + r.stderr
        return r.stdout.split()
    return run


def test_the_sweep_yields_the_25_bodies(traj_bodies):
    assert len(BODIES) == 25 == len(set(BODIES))
    keys = traj_bodies("sweep")
    assert "Unsupported" not in keys
    assert sorted(keys) == BODIES


def test_every_gpu_case_runs_the_body_written_beside_it(traj_bodies):
    args = []
    for K, side, n, kernel, _, steps, f32, _ in TABLE.values():
        assert len(steps) == n
        args += [side, K, int(f32), capi.KERNELS[kernel or "auto"], n]
    got = traj_bodies(*args)
    assert dict(zip(TABLE, got)) == {name: row[7] for name, row in TABLE.items()}
    # batch invariance runs a subset of the chains: the same body
    sub = []
    for K, side, n, kernel, _, _, f32, _ in TABLE.values():
        sub += [side, K, int(f32), capi.KERNELS[kernel or "auto"], min(n, 2)]
    assert traj_bodies(*sub) == got


def test_the_gpu_cases_cover_every_body():
    assert sorted({row[7] for row in TABLE.values()}) == BODIES
