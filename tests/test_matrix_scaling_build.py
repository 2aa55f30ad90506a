"""Build-time guard for the matrix-scaling head (no GPU needed: hipcc cross-compiles): tests/test_build_resources.py's check applied to
head_fused_mat.hip — every kernel keeps its accumulators in registers, ScratchSize 0 and no VGPR spill."""
import os
import re
import shutil
import subprocess

import pytest

from bayesnn_fpga_amd import _build


def test_matrix_head_kernels_have_no_scratch_and_no_spills():
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not available")
    r = subprocess.run([hipcc, *_build.FLAGS, "-Rpass-analysis=kernel-resource-usage", "-c", os.path.join(_build.CSRC, "head_fused_mat.hip"),
                        "-o", os.devnull], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    # (the remarks of one kernel come in this order: name, ..., ScratchSize, Occupancy, SGPRs Spill, VGPRs Spill)
    kernels = re.findall(r"Function Name: (\S+).*?ScratchSize \[bytes/lane\]: (\d+).*?VGPRs Spill: (\d+)", r.stderr, flags=re.S)
    assert len(kernels) == 120, len(kernels)       # 2 kernels x (RT 1, 2: 5 input kinds x 2 entropy forms; RT 3, 4: x 2 class-split forms)
    assert all("head_fused_mat_kernel" in n or "head_fused_multi_mat_kernel" in n for n, _, _ in kernels)
    bad = [(n, sc, sp) for n, sc, sp in kernels if int(sc) or int(sp)]
    assert not bad, f"kernels with scratch / VGPR spills: {bad}"
