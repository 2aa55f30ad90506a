"""Build-time guard for the rank-quality kernels (no GPU needed: hipcc cross-compiles): tests/test_reliability_kde_build.py's check applied
to ranking.hip — every kernel keeps its state in registers and LDS, ScratchSize 0 and no VGPR spill."""
import os
import re
import shutil
import subprocess

import pytest

from bayesnn_fpga_amd import _build


def test_ranking_kernels_have_no_scratch_and_no_spills():
    assert "ranking.hip" in _build.SOURCES
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not available")
    r = subprocess.run([hipcc, *_build.FLAGS, "-Rpass-analysis=kernel-resource-usage", "-c", os.path.join(_build.CSRC, "ranking.hip"),
                        "-o", os.devnull], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    kernels = re.findall(r"Function Name: (\S+).*?ScratchSize \[bytes/lane\]: (\d+).*?VGPRs Spill: (\d+)", r.stderr, flags=re.S)
    # the score keys, the pair counting (the hot path) and the per-row finish
    assert len(kernels) == 3, len(kernels)
    names = ("score_record", "rank_count", "rank_finish")
    assert sorted(next((k for k in names if f"{k}_kernel" in n), n) for n, _, _ in kernels) == sorted(names)
    bad = [(n, sc, sp) for n, sc, sp in kernels if int(sc) or int(sp)]
    assert not bad, f"kernels with scratch / VGPR spills: {bad}"
