"""Host side of the quantised multi-exit LeNet-5 (no GPU): the C ABI's three entry points and their refusals, the model's arguments."""
import ctypes as C

import pytest

from bayesnn_fpga_amd import _lib
from bayesnn_fpga_amd.models import extra as bx


def _create(W=6, I=0, out_dim=10, sites=(), null=False):
    buf = (C.c_double * 8)()
    desc = _lib.QLenet5MeDesc(*[None if null else C.addressof(buf)] * 14, out_dim, W, I)      # create is host-only and reads none of them
    for i, s in enumerate(sites):
        desc.sites[i] = s
    h = C.c_void_p()
    rc = _lib.lib().bmi_qlenet5_me_create(C.byref(desc), C.byref(h))
    if rc == 0:
        _lib.lib().bmi_qlenet5_me_destroy(h)
    return rc


def test_entry_points_and_refusals():
    for name in ("bmi_qlenet5_me_create", "bmi_qlenet5_me_forward_mcd", "bmi_qlenet5_me_destroy"):
        assert name in _lib.EXPORTS and hasattr(_lib.lib(), name)
    assert _lib.lib().bmi_version() == 600
    site = lambda kind, p: _lib.make_site(kind, 0, p, 4 if kind == _lib.SITE_MASKSEMBLE else 0)
    assert _create() == 0 and _create(2, 1) == 0 and _create(8, 7, 32, [site(_lib.SITE_NONE, 0.0), site(_lib.SITE_ELEMENTWISE, 0.0)]) == 0
    for W, I in ((1, 0), (9, 0), (6, 6), (6, -1)):
        assert _create(W, I) == -95, (W, I)
    assert _create(out_dim=33) == -95 and _create(out_dim=1) == -95
    assert _create(sites=[site(_lib.SITE_CHANNEL, 0.2)]) == -95 and _create(sites=[site(_lib.SITE_MASKSEMBLE, 0.0)]) == -95
    assert _create(sites=[site(_lib.SITE_ELEMENTWISE, 1.0)]) == -22
    assert _create(null=True) == -22 and _lib.lib().bmi_qlenet5_me_create(None, None) == -22
    assert _lib.lib().bmi_qlenet5_me_forward_mcd(None, None, 1, 0, 1, 0, None, None, None, None, None) == -22


def test_model_arguments():
    for W, I in ((1, 0), (9, 0), (6, 6), (6.0, 0)):
        with pytest.raises(ValueError):
            bx.LeNet5MCEarlyExit(quant_tbit=W, quant_ibit=I)
    m = bx.LeNet5MCEarlyExit(quant_tbit=6)
    assert (m.quant_tbit, m.quant_ibit, m.family, m.n_exits) == (6, 0, "lenet5_me", 2)
    assert list(m.state_dict()) == list(bx.LeNet5MCEarlyExit().state_dict())
    assert bx.LeNet5MCEarlyExit().quant_tbit is None
