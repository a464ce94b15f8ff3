"""CPU check of how librhmc_post's kernels compile for gfx950: the Makefile's
`resources` target prints the compiler's kernel-resource-usage remarks, and
every kernel must report 0 bytes of scratch (the lag ring and the per-lag sums
are statically indexed registers; a spill or a dynamically indexed private
array would show here)."""
import os
import re
import subprocess

import pytest

from conftest import PKG_DIR


@pytest.fixture(scope="module")
def remarks():
    if not os.path.exists("/opt/rocm/bin/hipcc") and "HIPCC" not in os.environ:
        pytest.skip("hipcc not available")
    r = subprocess.run(["make", "-C", os.path.join(PKG_DIR, "post"), "resources"],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    kernels, cur = {}, None
    for line in (r.stdout + r.stderr).splitlines():
        m = re.search(r"remark: Function Name: (\S+)", line)
        if m:
            cur = kernels.setdefault(m.group(1), {})
            continue
        m = re.search(r"remark:\s+([A-Za-z ]+?)(?: \[[^\]]*\])?: (\d+)", line)
        if m and cur is not None:
            cur[m.group(1).strip()] = int(m.group(2))
    return r.stdout + r.stderr, kernels


def test_resources_target_reports_gfx950_kernels(remarks):
    text, kernels = remarks
    assert "--offload-arch=gfx950" in text
    names = " ".join(kernels)
    for k in ("post_pass_kernel", "post_vario_reduce", "post_moment_reduce",
              "post_accept_kernel"):
        assert k in names, (k, sorted(kernels))
    # first and later pass of both lag-block sizes
    assert sum("post_pass_kernel" in k for k in kernels) == 4


def test_every_kernel_is_scratch_free(remarks):
    _, kernels = remarks
    assert kernels
    for name, res in kernels.items():
        assert "ScratchSize" in res and "VGPRs" in res, (name, res)
        assert res["ScratchSize"] == 0, "%s: %d bytes of scratch per lane" % (name,
                                                                               res["ScratchSize"])
        # wave64: one wave per SIMD at the least, whatever the registers
        assert res["Occupancy"] >= 1
