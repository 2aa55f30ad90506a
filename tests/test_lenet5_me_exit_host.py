"""Host side of the staged early exit of the fused multi-exit LeNet-5 (no GPU): the entry point and its refusals, all decided before any
HIP call, and the build-time resource guard of tests/test_lenet5_me_host.py for csrc/lenet5_me_exit.hip.  (A single-exit ``LeNet5Engine``
raising needs an engine, so a device: tests/test_lenet5_me_exit.py.)"""
import ctypes as C
import os
import re
import shutil
import subprocess

import pytest

from bayesnn_fpga_amd import _build, _lib

NAME = "bmi_lenet5_me_forward_exit_staged"


def test_entry_point_is_exported():
    assert NAME in _lib.EXPORTS and hasattr(_lib.lib(), NAME)


# (argument that is wrong, return code); arguments: handle, x, batch, t_count, seed, rule, S1, S2, SL, exit_of_image, stream
@pytest.mark.parametrize("bad,rc", [("handle", -22), ("x", -22), ("rule", -22), ("S1", -22), ("S2", -22), ("SL", -22), ("exit_of_image", -22),
                                    ("batch", -22), ("t_count", -22), ("criterion", -22), ("first_exit", -22), ("ensemble", -95)])
def test_refusals_before_any_hip_call(bad, rc):
    buf = (C.c_double * 8)()
    desc = _lib.Lenet5MeDesc(*[C.addressof(buf)] * 14, 10)      # non-null addresses: create is host-only and reads none of them
    h = C.c_void_p()
    assert _lib.lib().bmi_lenet5_me_create(C.byref(desc), C.byref(h)) == 0
    rule = _lib.ExitRule(7 if bad == "criterion" else 0, int(bad == "ensemble"), 0.5, int(bad == "first_exit"))
    ptr = lambda name: None if bad == name else C.addressof(buf)
    try:
        got = getattr(_lib.lib(), NAME)(None if bad == "handle" else h, ptr("x"), 0 if bad == "batch" else 1, 0 if bad == "t_count" else 1, 0,
                                        None if bad == "rule" else C.byref(rule), ptr("S1"), ptr("S2"), ptr("SL"), ptr("exit_of_image"), None)
    finally:
        _lib.lib().bmi_lenet5_me_destroy(h)
    assert got == rc


def test_kernel_fits_two_workgroups_per_cu_without_scratch_or_spills():
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not available")
    assert "lenet5_me_exit.hip" in _build.SOURCES
    r = subprocess.run([hipcc, *_build.FLAGS, *_build.EXTRA_FLAGS["lenet5_me_exit.hip"], "-Rpass-analysis=kernel-resource-usage", "-c",
                        os.path.join(_build.CSRC, "lenet5_me_exit.hip"), "-o", os.devnull], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    blocks = r.stderr.split("Function Name: ")[1:]          # one block of remarks per kernel
    num = lambda blk, what: int(re.search(re.escape(what) + r": (\d+)", blk).group(1))
    kernels = [(blk.split()[0], num(blk, "VGPRs"), num(blk, "VGPRs Spill"), num(blk, "ScratchSize [bytes/lane]"), num(blk, "LDS Size [bytes/block]"))
               for blk in blocks]
    assert [k[0] for k in kernels if "lenet5_me_exit_kernel" in k[0]], kernels
    assert not [k for k in kernels if k[1] > 256 or k[2] or k[3] or k[4] > 81920], kernels
