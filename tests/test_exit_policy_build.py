"""Build-time guard for the exit-policy kernels (no GPU needed: hipcc cross-compiles): tests/test_ranking_build.py's check applied to
exit_policy.hip — every kernel keeps its state in registers and LDS, ScratchSize 0 and no VGPR spill (the sweep keeps an image's valid and
hit bits as two masks, not as an array indexed by the exit)."""
import os
import re
import shutil
import subprocess

import pytest

from bayesnn_fpga_amd import _build


def test_exit_policy_kernels_have_no_scratch_and_no_spills():
    assert "exit_policy.hip" in _build.SOURCES
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not available")
    r = subprocess.run([hipcc, *_build.FLAGS, "-Rpass-analysis=kernel-resource-usage", "-c", os.path.join(_build.CSRC, "exit_policy.hip"),
                        "-o", os.devnull], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    kernels = re.findall(r"Function Name: (\S+).*?ScratchSize \[bytes/lane\]: (\d+).*?VGPRs Spill: (\d+)", r.stderr, flags=re.S)
    # the statistic record, the sweep (the hot path) and the sum of its partial counts
    assert len(kernels) == 3, len(kernels)
    names = ("exit_stat_record", "exit_policy_sweep", "exit_policy_finish")
    assert sorted(next((k for k in names if f"{k}_kernel" in n), n) for n, _, _ in kernels) == sorted(names)
    bad = [(n, sc, sp) for n, sc, sp in kernels if int(sc) or int(sp)]
    assert not bad, f"kernels with scratch / VGPR spills: {bad}"
