"""Host side of the quantised LeNet-5 (no GPU): the two quantisers against direct arithmetic, the C ABI's refusals, the model's arguments."""
import ctypes as C

import pytest
import torch

from bayesnn_fpga_amd import _lib
from bayesnn_fpga_amd.models import extra as bx
from bayesnn_fpga_amd.quant import act_codes, weight_codes


@pytest.mark.parametrize("W,I", [(6, 0), (8, 0), (8, 3), (2, 0), (8, 7)])
def test_quantisers_round_half_to_even_and_clip(W, I):
    s, lo, hi = 2.0 ** (W - 1 - I), -2 ** (W - 1), 2 ** (W - 1) - 1
    # ties on both sides of zero (to the even neighbour), an ordinary value, both clip ends and beyond
    q = [0.5, 1.5, 2.5, -0.5, -1.5, 0.3, -0.7, hi, hi + 0.5, hi + 40, lo, lo - 0.5, lo - 40]
    want = [0, 2, 2, 0, -2, 0, -1, hi, hi, hi, lo, lo, lo]
    assert weight_codes(torch.tensor(q, dtype=torch.float64) / s, W, I).tolist() == [min(max(v, lo), hi) for v in want]
    top = 2 ** W - 1
    a = [0.5, 1.5, 2.5, 0.3, -0.5, -3.0, top - 0.5, top, top + 0.5, top + 9]
    assert act_codes(torch.tensor(a, dtype=torch.float64) / 2.0 ** W, W).tolist() == [0, 2, 2, 0, 0, 0, top - 1 if top % 2 else top, top, top, top]


def _create(W=6, I=0, out_dim=10, sites=(), null=False):
    buf = (C.c_double * 8)()
    desc = _lib.QLenet5Desc(*[None if null else C.addressof(buf)] * 8, out_dim, W, I)      # create is host-only and reads none of them
    for i, s in enumerate(sites):
        desc.sites[i] = s
    h = C.c_void_p()
    rc = _lib.lib().bmi_qlenet5_create(C.byref(desc), C.byref(h))
    if rc == 0:
        _lib.lib().bmi_qlenet5_destroy(h)
    return rc


def test_entry_points_and_refusals():
    for name in ("bmi_qlenet5_create", "bmi_qlenet5_forward_mcd", "bmi_qlenet5_destroy"):
        assert name in _lib.EXPORTS and hasattr(_lib.lib(), name)
    assert _lib.lib().bmi_version() == 600
    site = lambda kind, p: _lib.make_site(kind, 0, p, 4 if kind == _lib.SITE_MASKSEMBLE else 0)
    assert _create() == 0 and _create(2, 1) == 0 and _create(8, 7, 32, [site(_lib.SITE_ELEMENTWISE, 0.0)]) == 0
    for W, I in ((1, 0), (9, 0), (6, 6), (6, -1)):
        assert _create(W, I) == -95, (W, I)
    assert _create(out_dim=33) == -95 and _create(out_dim=1) == -95
    assert _create(sites=[site(_lib.SITE_CHANNEL, 0.2)]) == -95 and _create(sites=[site(_lib.SITE_MASKSEMBLE, 0.0)]) == -95
    assert _create(sites=[site(_lib.SITE_ELEMENTWISE, 1.0)]) == -22
    assert _create(null=True) == -22 and _lib.lib().bmi_qlenet5_create(None, None) == -22
    assert _lib.lib().bmi_qlenet5_forward_mcd(None, None, 1, 0, 1, 0, None, None, None, None, None) == -22


def test_model_arguments():
    with pytest.raises(ValueError):
        bx.LeNet5MC(quant_tbit=6, mask_type="mask")
    for W, I in ((1, 0), (9, 0), (6, 6)):
        with pytest.raises(ValueError):
            bx.LeNet5MC(quant_tbit=W, quant_ibit=I)
    assert list(bx.LeNet5MC(quant_tbit=6).state_dict()) == list(bx.LeNet5MC().state_dict())
    assert bx.LeNet5MC().quant_tbit is None
