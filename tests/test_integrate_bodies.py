"""Which kernel body serves an explicit integrator, on the CPU.

tests/native/traj_bodies.cpp in its `integrate` mode (a host compiler,
csrc/rhmc_select.hpp and csrc/rhmc_dispatch.hpp alone) names the body that
rhmc_integrate launches for a shape under RHMC_SOLVER_HMC, _RHMC_NAIVE or
_RHMC_LEAPFROG, by calling the switches of rhmc_dispatch.hpp that
launch_integrate (csrc/rhmc_launch.hpp) calls.  Op::Integrate shares its
row of op_rules() with Op::HmcRandom, so the bodies are the 25 of
test_traj_bodies.BODIES, each built once per solver:

* the sweep (sides 32/48/64/96, K = 1..1024, fp32-exact or not, every
  RHMC_KERNEL_* value, 4 and 65536 chains) yields exactly these 25 and never
  an unsupported plan,
* every case of tests/test_gpu_integrate_bodies.py's TABLE runs the body
  written beside it, at every chain count the GPU tests launch, and the table
  covers all 25.

The day the two ops stop sharing their rules, or a threshold moves, this fails
until a GPU case covers the integrators' bodies again."""
from rhmc_amd import capi
from test_gpu_integrate_bodies import TABLE
from test_traj_bodies import BODIES, traj_bodies  # noqa: F401 (the fixture)


def test_the_integrate_sweep_yields_the_25_bodies(traj_bodies):
    assert len(BODIES) == 25 == len(set(BODIES))
    keys = traj_bodies("integrate", "sweep")
    assert "Unsupported" not in keys
    assert sorted(keys) == BODIES


def test_every_gpu_case_runs_the_body_written_beside_it(traj_bodies):
    want = {name: row[5] for name, row in TABLE.items()}
    # all chains; the even and the odd chains (the wall launches); the batch-
    # invariance subsets of those, two chains or one
    counts = (lambda n: n, lambda n: (n + 1) // 2, lambda n: n // 2, lambda n: min(n, 2),
              lambda n: 1)
    for count in counts:
        args = []
        for K, side, n, kernel, f32, _, _, _, n_steps in TABLE.values():
            assert n >= 2 and n_steps >= 1
            args += [side, K, int(f32), capi.KERNELS[kernel or "auto"], count(n)]
        assert dict(zip(TABLE, traj_bodies("integrate", *args))) == want


def test_the_gpu_cases_cover_every_body():
    assert sorted({row[5] for row in TABLE.values()}) == BODIES
