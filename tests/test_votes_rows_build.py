"""Build-time guard for the image-list vote kernels (no GPU needed: hipcc cross-compiles): tests/test_votes_build.py's check applied to
votes_rows.hip — every instantiation of the rows count kernel (four maps x plain / weighted) and the two forms of the decide kernel keep
their state in registers, ScratchSize 0 and no VGPR spill."""
import os
import re
import shutil
import subprocess

import pytest

from bayesnn_fpga_amd import _build


def test_vote_rows_kernels_have_no_scratch_and_no_spills():
    assert "votes_rows.hip" in _build.SOURCES
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not available")
    r = subprocess.run([hipcc, *_build.FLAGS, "-Rpass-analysis=kernel-resource-usage", "-c", os.path.join(_build.CSRC, "votes_rows.hip"),
                        "-o", os.devnull], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    # (the remarks of one kernel come in this order: name, ..., ScratchSize, Occupancy, SGPRs Spill, VGPRs Spill)
    kernels = re.findall(r"Function Name: (\S+).*?ScratchSize \[bytes/lane\]: (\d+).*?VGPRs Spill: (\d+)", r.stderr, flags=re.S)
    names = [n for n, _, _ in kernels]
    assert len(kernels) == 10, names               # vote_counts_rows_kernel<map 0..3, weighted 0 | 1> and vote_decide_kernel<final 0 | 1>
    assert sum("vote_counts_rows_kernel" in n for n in names) == 8 and sum("vote_decide_kernel" in n for n in names) == 2
    assert len(set(names)) == 10
    bad = [(n, sc, sp) for n, sc, sp in kernels if int(sc) or int(sp)]
    assert not bad, f"kernels with scratch / VGPR spills: {bad}"
