"""Kernel selection (csrc/rhmc_select.hpp) on the CPU: the header is plain
C++17 with no HIP include, so tests/native/select_check.cpp is built with a
host compiler alone and asserts the plan for the configurations the project's
documents name: the README workloads (C1/C2, C3, C5, B4), the thresholds of
DESIGN.md section 4 (lane-group batch sizes, dense from 11 stars, global
tables from 65, window split), every RHMC_KERNEL_* value of include/rhmc.h,
the PSF-width limit and the ragged families."""
import os
import shutil
import subprocess

import pytest

from conftest import PKG_DIR, ROOT


def test_select_plans_match_the_documents(tmp_path):
    gxx = shutil.which("g++")
    if not gxx:
        pytest.skip("g++ not available")
    exe = str(tmp_path / "select_check")
    subprocess.run([gxx, "-std=c++17", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"),
                    "-I", os.path.join(PKG_DIR, "csrc"), "-o", exe,
                    os.path.join(ROOT, "tests", "native", "select_check.cpp")], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "select ok" in r.stdout
