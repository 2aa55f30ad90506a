"""Build-time guard for the per-pass accuracy read-out (no GPU needed: hipcc cross-compiles): tests/test_matrix_scaling_build.py's check
applied to pass_accuracy.hip — both kernels keep their state in registers, ScratchSize 0 and no VGPR spill."""
import os
import re
import shutil
import subprocess

import pytest

from bayesnn_fpga_amd import _build


def test_pass_accuracy_kernels_have_no_scratch_and_no_spills():
    assert "pass_accuracy.hip" in _build.SOURCES
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not available")
    r = subprocess.run([hipcc, *_build.FLAGS, "-Rpass-analysis=kernel-resource-usage", "-c", os.path.join(_build.CSRC, "pass_accuracy.hip"),
                        "-o", os.devnull], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    # (the remarks of one kernel come in this order: name, ..., ScratchSize, Occupancy, SGPRs Spill, VGPRs Spill)
    kernels = re.findall(r"Function Name: (\S+).*?ScratchSize \[bytes/lane\]: (\d+).*?VGPRs Spill: (\d+)", r.stderr, flags=re.S)
    assert len(kernels) == 2, len(kernels)         # the per-(pass, image) rows kernel and the per-(pass, exit) reduction
    assert sorted("rows" if "pass_accuracy_rows_kernel" in n else "reduce" if "pass_accuracy_reduce_kernel" in n else n for n, _, _ in kernels) == \
        ["reduce", "rows"]
    bad = [(n, sc, sp) for n, sc, sp in kernels if int(sc) or int(sp)]
    assert not bad, f"kernels with scratch / VGPR spills: {bad}"
