"""Build-time guard for the vote kernels (no GPU needed: hipcc cross-compiles): tests/test_pass_accuracy_build.py's check applied to
votes.hip — every instantiation of the count kernel (four maps x plain / weighted) and the read-out keep their state in registers,
ScratchSize 0 and no VGPR spill."""
import os
import re
import shutil
import subprocess

import pytest

from bayesnn_fpga_amd import _build


def test_vote_kernels_have_no_scratch_and_no_spills():
    assert "votes.hip" in _build.SOURCES
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not available")
    r = subprocess.run([hipcc, *_build.FLAGS, "-Rpass-analysis=kernel-resource-usage", "-c", os.path.join(_build.CSRC, "votes.hip"),
                        "-o", os.devnull], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    # (the remarks of one kernel come in this order: name, ..., ScratchSize, Occupancy, SGPRs Spill, VGPRs Spill)
    kernels = re.findall(r"Function Name: (\S+).*?ScratchSize \[bytes/lane\]: (\d+).*?VGPRs Spill: (\d+)", r.stderr, flags=re.S)
    names = [n for n, _, _ in kernels]
    assert len(kernels) == 9, names                # vote_counts_kernel<map 0..3, weighted 0 | 1> and finalize_votes_kernel
    assert sum("vote_counts_kernel" in n for n in names) == 8 and sum("finalize_votes_kernel" in n for n in names) == 1
    assert len(set(names)) == 9
    bad = [(n, sc, sp) for n, sc, sp in kernels if int(sc) or int(sp)]
    assert not bad, f"kernels with scratch / VGPR spills: {bad}"
