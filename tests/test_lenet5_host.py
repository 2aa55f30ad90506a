"""Host side of the fused LeNet-5 (no GPU): the mirror against the oracle's restatement, the C ABI's three entry points and their
refusals, and the build-time resource guard of tests/test_build_resources.py for csrc/lenet5.hip."""
import ctypes as C
import os
import re
import shutil
import subprocess

import pytest
import torch

from bayesnn_fpga_amd import _build, _lib
from bayesnn_fpga_amd.models import extra as bx
from oracle import extra_models as ox
from tests.helpers import build_seeded, state_checksum


def test_mirror_matches_the_oracle_and_has_no_cpu_forward():
    kw = dict(dropout_p=0.2, out_dim=10)
    a, b = build_seeded(bx.LeNet5MC, kw), build_seeded(ox.LeNet5MC, kw)
    assert list(a.state_dict()) == list(b.state_dict())
    assert state_checksum(a.state_dict()) == state_checksum(b.state_dict())
    with pytest.raises(RuntimeError, match="no CPU"):
        a(torch.zeros(1, 1, 28, 28))


@pytest.mark.parametrize("k", [0, 1, 2, 3])
def test_site_counter_rule(k):
    """models.py:36-68 with three candidate sites: the last k are on, numbered in call order."""
    m = bx.LeNet5MC(num_bayes_layer=k)
    assert sum(isinstance(x, torch.nn.Dropout) for x in m.modules()) == k
    sites = m.site_descs()
    assert [s.kind for s in sites] == [_lib.SITE_NONE] * (3 - k) + [_lib.SITE_ELEMENTWISE] * k
    assert [s.site_id for s in sites if s.kind] == list(range(k))


def _create(out_dim=10, sites=()):
    buf = (C.c_double * 8)()
    desc = _lib.Lenet5Desc(*[C.addressof(buf)] * 8, out_dim)      # non-null addresses: create is host-only and reads none of them
    for i, s in enumerate(sites):
        desc.sites[i] = s
    h = C.c_void_p()
    rc = _lib.lib().bmi_lenet5_create(C.byref(desc), C.byref(h))
    if rc == 0:
        _lib.lib().bmi_lenet5_destroy(h)
    return rc


def test_entry_points_and_refusals():
    for name in ("bmi_lenet5_create", "bmi_lenet5_forward_mcd", "bmi_lenet5_destroy"):
        assert name in _lib.EXPORTS and hasattr(_lib.lib(), name)
    assert _lib.lib().bmi_version() == 600
    site = lambda kind, p: _lib.make_site(kind, 0, p)
    assert _create() == 0 and _create(32, [site(_lib.SITE_ELEMENTWISE, 0.0)]) == 0
    assert _create(33) == -95 and _create(1) == -95
    assert _create(sites=[site(_lib.SITE_CHANNEL, 0.2)]) == -95
    assert _create(sites=[site(_lib.SITE_ELEMENTWISE, 1.0)]) == -22
    assert _lib.lib().bmi_lenet5_forward_mcd(None, None, 1, 0, 1, 0, None, None, None, None, None) == -22


def test_lenet5_kernels_have_no_scratch_and_no_spills():
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not available")
    assert "lenet5.hip" in _build.SOURCES
    r = subprocess.run([hipcc, *_build.FLAGS, *_build.EXTRA_FLAGS["lenet5.hip"], "-Rpass-analysis=kernel-resource-usage", "-c",
                        os.path.join(_build.CSRC, "lenet5.hip"), "-o", os.devnull], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    blocks = r.stderr.split("Function Name: ")[1:]          # one block of remarks per kernel (ScratchSize stands in front of VGPRs Spill)
    kernels = [(blk.split()[0], int(re.search(r"VGPRs Spill: (\d+)", blk).group(1)), int(re.search(r"ScratchSize \[bytes/lane\]: (\d+)", blk).group(1)))
               for blk in blocks]
    assert len(kernels) == 2, kernels
    assert not [k for k in kernels if k[1] or k[2]], kernels
