"""Build-time guard for the reliability kernels (no GPU needed: hipcc cross-compiles): tests/test_pass_accuracy_build.py's check applied to
reliability.hip — every kernel keeps its state in registers and LDS, ScratchSize 0 and no VGPR spill."""
import os
import re
import shutil
import subprocess

import pytest

from bayesnn_fpga_amd import _build


def test_reliability_kernels_have_no_scratch_and_no_spills():
    assert "reliability.hip" in _build.SOURCES
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not available")
    r = subprocess.run([hipcc, *_build.FLAGS, "-Rpass-analysis=kernel-resource-usage", "-c", os.path.join(_build.CSRC, "reliability.hip"),
                        "-o", os.devnull], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    # (the remarks of one kernel come in this order: name, ..., ScratchSize, Occupancy, SGPRs Spill, VGPRs Spill)
    kernels = re.findall(r"Function Name: (\S+).*?ScratchSize \[bytes/lane\]: (\d+).*?VGPRs Spill: (\d+)", r.stderr, flags=re.S)
    # the per-image records kernel, the per-(line, edge) radix select (shared with the classwise table: line_edges_kernel), the
    # per-(chunk, row) integer bins and the per-row finish
    assert len(kernels) == 4, len(kernels)
    names = ("reliability_records", "line_edges", "reliability_partial", "reliability_bins")
    assert sorted(next((k for k in names if f"{k}_kernel" in n), n) for n, _, _ in kernels) == sorted(names)
    bad = [(n, sc, sp) for n, sc, sp in kernels if int(sc) or int(sp)]
    assert not bad, f"kernels with scratch / VGPR spills: {bad}"
