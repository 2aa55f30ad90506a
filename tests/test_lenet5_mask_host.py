"""Host side of the Masksembles LeNet-5 (no GPU): what ``bmi_lenet5_create`` takes and refuses, the mirror's modules and site descriptors,
and the build-time resource guard of tests/test_lenet5_host.py for csrc/lenet5_mask.hip."""
import ctypes as C
import os
import re
import shutil
import subprocess

import pytest

from bayesnn_fpga_amd import _build, _lib
from bayesnn_fpga_amd.models import extra as bx
from bayesnn_fpga_amd.models.resnet18.resnet18 import MCDropout
from bayesnn_fpga_amd.utils import Masksembles1D, Masksembles2D

BUF = (C.c_double * 8)()
PTR = C.addressof(BUF)          # a non-null address: create is host-only and reads none of them
MASK = lambda n=4, ptr=PTR: _lib.make_site(_lib.SITE_MASKSEMBLE, 0, 0.0, n, ptr)
MC = _lib.make_site(_lib.SITE_ELEMENTWISE, 0, 0.2)
OFF = _lib.make_site()


def create(sites, desc_type=_lib.Lenet5Desc, name="bmi_lenet5"):
    desc = desc_type(*[PTR] * (14 if name == "bmi_lenet5_me" else 8), 10)
    for i, s in enumerate(sites):
        desc.sites[i] = s
    h = C.c_void_p()
    rc = getattr(_lib.lib(), name + "_create")(C.byref(desc), C.byref(h))
    if rc == 0:
        getattr(_lib.lib(), name + "_destroy")(h)
    return rc


@pytest.mark.parametrize("k", [1, 2, 3])
def test_create_takes_masksembles_sites(k):
    assert create([OFF] * (3 - k) + [MASK()] * k) == 0 and _lib.lib().bmi_version() == 600
    assert create([MASK(), MASK()], _lib.Lenet5MeDesc, "bmi_lenet5_me") == -95      # the multi-exit form still refuses


@pytest.mark.parametrize("sites,rc", [
    ([MC, MASK(), MASK()], -95), ([OFF, MASK(), MC], -95),          # MC dropout and Masksembles in one model
    ([MASK(4), MASK(3), MASK(4)], -95),                             # unequal num_masks
    ([OFF, OFF, MASK(4, None)], -22),                               # no masks
    ([OFF, OFF, MASK(0)], -22), ([OFF, OFF, MASK(-1)], -22),        # num_masks < 1
    ([OFF, OFF, MASK(33)], -95), ([OFF, OFF, MASK(32)], 0),         # num_masks > 32
    ([OFF, OFF, _lib.make_site(_lib.SITE_CHANNEL, 0, 0.2)], -95),   # channelwise sites stay unsupported
])
def test_create_refusals(sites, rc):
    assert create(sites) == rc


@pytest.mark.parametrize("k", [0, 1, 2, 3])
def test_mirror(k):
    m = bx.LeNet5MC(num_bayes_layer=k, mask_type="mask", num_masks=3)
    want = [("drop_a", Masksembles2D, 20), ("drop_b", Masksembles1D, 80), ("drop", Masksembles1D, 100)][3 - k:]
    assert [(n, type(x), x.channels, x.n) for n, x in m.named_modules() if n.startswith("drop")] == [(n, t, c, 3) for n, t, c in want]
    assert [s.kind for s in m.site_descs()] == [_lib.SITE_NONE] * (3 - k) + [_lib.SITE_MASKSEMBLE] * k
    assert [(s.num_masks, s.masks) for s in m.site_descs([PTR] * 3) if s.kind] == [(3, PTR)] * k
    plain = bx.LeNet5MC(num_bayes_layer=k)
    assert set(m.state_dict()) - set(plain.state_dict()) == {n + ".masks" for n, _, _ in want} and set(plain.state_dict()) <= set(m.state_dict())
    assert plain.mask_type == "mc" and not plain.mask_layers() and [type(x) for x in plain.site_mods() if x is not None] == [MCDropout] * k
    assert [s.kind for s in plain.site_descs()] == [_lib.SITE_NONE] * (3 - k) + [_lib.SITE_ELEMENTWISE] * k


def test_lenet5_mask_kernels_have_no_scratch_and_no_spills():
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not available")
    assert "lenet5_mask.hip" in _build.SOURCES
    r = subprocess.run([hipcc, *_build.FLAGS, *_build.EXTRA_FLAGS["lenet5_mask.hip"], "-Rpass-analysis=kernel-resource-usage", "-c",
                        os.path.join(_build.CSRC, "lenet5_mask.hip"), "-o", os.devnull], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    blocks = r.stderr.split("Function Name: ")[1:]          # one block of remarks per kernel (ScratchSize stands in front of VGPRs Spill)
    kernels = [(blk.split()[0], int(re.search(r"VGPRs Spill: (\d+)", blk).group(1)), int(re.search(r"ScratchSize \[bytes/lane\]: (\d+)", blk).group(1)))
               for blk in blocks]
    assert len(kernels) == 2, kernels
    assert not [k for k in kernels if k[1] or k[2]], kernels
