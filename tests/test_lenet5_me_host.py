"""Host side of the fused multi-exit LeNet-5 (no GPU): the mirror's parameters and sites, the C ABI's three entry points and their
refusals, and the build-time resource guard of tests/test_lenet5_host.py for csrc/lenet5_me.hip."""
import ctypes as C
import os
import re
import shutil
import subprocess

import pytest
import torch

from bayesnn_fpga_amd import _build, _lib
from bayesnn_fpga_amd.models import extra as bx


def test_mirror_extends_the_single_exit_trunk_and_has_no_cpu_forward():
    m = bx.LeNet5MCEarlyExit()
    trunk = bx.LeNet5MC().state_dict()
    branch = [f"{mod}.{p}" for mod in ("ex1conv1", "ex1fc1", "ex1linear") for p in ("weight", "bias")]
    assert sorted(m.state_dict()) == sorted(list(trunk) + branch)
    assert (m.family, m.multi_exit, m.n_exits) == ("lenet5_me", True, 2)
    assert tuple(m.ex1conv1.weight.shape) == (20, 20, 5, 5) and m.ex1conv1.stride == (7, 7) and m.ex1conv1.padding == (0, 0)
    missing, unexpected = m.load_state_dict(trunk, strict=False)
    assert sorted(missing) == sorted(branch) and not unexpected and torch.equal(m.fc2.weight, trunk["fc2.weight"])
    with pytest.raises(RuntimeError, match="no CPU"):
        m(torch.zeros(1, 1, 28, 28))


@pytest.mark.parametrize("dropout_exit", [True, False])
def test_sites(dropout_exit):
    sites = bx.LeNet5MCEarlyExit(dropout_exit=dropout_exit, dropout_p=0.25).site_descs()
    assert [s.kind for s in sites] == [_lib.SITE_ELEMENTWISE if dropout_exit else _lib.SITE_NONE] * 2
    assert [(s.site_id, s.p) for s in sites if s.kind] == ([(0, 0.25), (1, 0.25)] if dropout_exit else [])      # early exit, then main exit


def _create(out_dim=10, sites=()):
    buf = (C.c_double * 8)()
    desc = _lib.Lenet5MeDesc(*[C.addressof(buf)] * 14, out_dim)      # non-null addresses: create is host-only and reads none of them
    for i, s in enumerate(sites):
        desc.sites[i] = s
    h = C.c_void_p()
    rc = _lib.lib().bmi_lenet5_me_create(C.byref(desc), C.byref(h))
    if rc == 0:
        _lib.lib().bmi_lenet5_me_destroy(h)
    return rc


def test_entry_points_and_refusals():
    for name in ("bmi_lenet5_me_create", "bmi_lenet5_me_forward_mcd", "bmi_lenet5_me_destroy"):
        assert name in _lib.EXPORTS and hasattr(_lib.lib(), name)
    site = lambda kind, p: _lib.make_site(kind, 0, p)
    assert _create() == 0 and _create(32, [site(_lib.SITE_NONE, 0.0), site(_lib.SITE_ELEMENTWISE, 0.0)]) == 0
    assert _create(33) == -95 and _create(1) == -95
    assert _create(sites=[site(_lib.SITE_CHANNEL, 0.2)]) == -95
    assert _create(sites=[site(_lib.SITE_ELEMENTWISE, 1.0)]) == -22
    assert _lib.lib().bmi_lenet5_me_forward_mcd(None, None, 1, 0, 1, 0, None, None, None, None, None) == -22


def test_kernel_fits_two_workgroups_per_cu_without_scratch_or_spills():
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not available")
    assert "lenet5_me.hip" in _build.SOURCES
    r = subprocess.run([hipcc, *_build.FLAGS, *_build.EXTRA_FLAGS["lenet5_me.hip"], "-Rpass-analysis=kernel-resource-usage", "-c",
                        os.path.join(_build.CSRC, "lenet5_me.hip"), "-o", os.devnull], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    blocks = r.stderr.split("Function Name: ")[1:]          # one block of remarks per kernel
    num = lambda blk, what: int(re.search(re.escape(what) + r": (\d+)", blk).group(1))
    kernels = [(blk.split()[0], num(blk, "VGPRs"), num(blk, "VGPRs Spill"), num(blk, "ScratchSize [bytes/lane]"), num(blk, "LDS Size [bytes/block]"))
               for blk in blocks]
    assert [k[0] for k in kernels if "lenet5_me_kernel" in k[0]], kernels
    assert not [k for k in kernels if k[1] > 256 or k[2] or k[3] or k[4] > 81920], kernels
