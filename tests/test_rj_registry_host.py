"""The owner of the native reversible-jump driver's per-(device, pipe) buffers
(hmc-stellar-toy-model_amd/host/rj_registry.hpp) without a GPU:
`make -C hmc-stellar-toy-model_amd/host registry_check` builds
tests/native/rj_registry_check.cpp twice, under -fsanitize=thread and under
-fsanitize=address.  Four threads lease pipes while a fifth releases them; the
program checks that every payload is destroyed exactly once after its last
use, that no lease holds a payload while it is destroyed, and that the map is
empty at the end.  A lock-order mistake is a deadlock: the timeout is that
assertion."""
import os
import subprocess

from conftest import PKG_DIR, ROOT

import pytest

HOST = os.path.join(PKG_DIR, "host")


def _run(kind):
    exe = os.path.join(ROOT, "build", kind, "rj_registry_check")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert "rj registry ok" in r.stdout
    assert "Sanitizer" not in r.stderr, r.stderr[-3000:]


def test_registry_lock_order_and_lifetimes_under_sanitizers():
    subprocess.run(["make", "-C", HOST, "registry_check_asan"], check=True, capture_output=True)
    _run("asan")
    b = subprocess.run(["make", "-C", HOST, "registry_check_tsan"], capture_output=True, text=True)
    if b.returncode != 0 and "tsan" in b.stderr and ("cannot find" in b.stderr
                                                     or "No such file" in b.stderr):
        pytest.skip("thread-sanitizer runtime not linkable: " + b.stderr.strip()[-400:])
    assert b.returncode == 0, b.stderr[-3000:]
    _run("tsan")
