"""CPU-side checks of adaptive Monte-Carlo sampling (bmi_forward_mcd_adaptive, bmi_finalize_per_image, MCDEngine.predict_adaptive):
every bad argument gets its return code before any launch.  The graphs live on the CPU, so a call that got as far as a launch would
fail with a HIP error instead."""
import ctypes as C

import numpy as np
import pytest

from bayesnn_fpga_amd import _lib
from bayesnn_fpga_amd.engine import CompiledGraph
from bayesnn_fpga_amd.models.resnet18.resnet18 import ResNet18MCEarlyExit
from tests.helpers import build_seeded

KW = dict(dropout_exit=True, dropout="block", dropout_p=0.25, out_dim=10)


def _graph(dtype="f16", max_batch=8, chunk=4):
    return CompiledGraph(build_seeded(ResNet18MCEarlyExit, KW), "cpu", max_batch, chunk, dtype=dtype)


def test_adaptive_entry_point_checks_arguments_before_any_launch():
    cg = _graph()
    lib, h, ws_ok, E = _lib.lib(), cg.handle, cg.workspace_bytes, cg.n_exits
    buf = np.zeros(64, dtype=np.float64)                  # a non-null address; no row gets far enough to use it
    p = buf.ctypes.data
    act = (C.c_int32 * 64)()

    def ad(h=h, x=p, batch=8, off=0, t_max=8, t_step=4, cnt0=0, rule=0, test_exit=3, S1=p, S2=p, SL=p, SH=p, t_used=p, conv=p, act=act,
           ws=p, nbytes=ws_ok):
        return lib.bmi_forward_mcd_adaptive(h, x, batch, off, t_max, t_step, 7, cnt0, rule, 0.01, test_exit, S1, S2, SL, SH, t_used, conv,
                                            act, ws, nbytes, None)

    small = ws_ok - 1
    rows = [
        (ad(h=None), -22), (ad(x=None), -22), (ad(S1=None), -22), (ad(S2=None), -22), (ad(SL=None), -22), (ad(t_used=None), -22),
        (ad(act=None), -22), (ad(ws=None), -22), (ad(off=-1), -22), (ad(off=-1, nbytes=small), -22),
        (ad(batch=0), -22), (ad(t_max=0), -22), (ad(t_step=0), -22), (ad(t_step=-3), -22), (ad(cnt0=-1), -22),
        (ad(rule=2), -22), (ad(rule=-1), -22), (ad(test_exit=-1), -22), (ad(test_exit=E), -22), (ad(batch=9), -22),
        (ad(batch=9, nbytes=small), -22), (ad(rule=5, t_step=5), -22), (ad(t_max=0, nbytes=small), -22),
        (ad(t_step=5), -95), (ad(t_step=5, nbytes=small), -95), (ad(nbytes=small), -12),
        (ad(SH=None, conv=None, nbytes=small), -12),         # the optional outputs: NULL is allowed
        (ad(t_max=3, t_step=4, nbytes=small), -12),          # T_max < t_step is allowed
    ]
    assert [rc for rc, _ in rows] == [want for _, want in rows]


def test_adaptive_refuses_the_exact_engine():
    cg = _graph("f32")
    lib = _lib.lib()
    buf = np.zeros(64, dtype=np.float64)
    p = buf.ctypes.data
    act = (C.c_int32 * 8)()
    rc = lib.bmi_forward_mcd_adaptive(cg.handle, p, 8, 0, 8, 4, 7, 0, 0, 0.01, 3, p, p, p, None, p, None, act, p, cg.workspace_bytes, None)
    assert rc == -95
    rc = lib.bmi_forward_mcd_adaptive(cg.handle, p, 8, 0, 8, 4, 7, 0, 0, 0.01, 3, p, p, p, None, p, None, act, p, cg.workspace_bytes - 1,
                                      None)
    assert rc == -95


def test_finalize_per_image_checks_arguments_before_any_launch():
    lib = _lib.lib()
    buf = np.zeros(64, dtype=np.float64)
    p = buf.ctypes.data

    def fin(E=4, B=8, Cd=10, t_used=p, S1=p, S2=p, SL=p, SH=None, mean=p, var=p, lm=p, pe=None, ee=None, mi=None):
        return lib.bmi_finalize_per_image(E, B, Cd, t_used, S1, S2, SL, SH, mean, var, lm, pe, ee, mi, None, None)

    rows = [
        (fin(t_used=None), -22), (fin(S1=None), -22), (fin(S2=None), -22), (fin(SL=None), -22), (fin(mean=None), -22),
        (fin(var=None), -22), (fin(lm=None), -22), (fin(E=0), -22), (fin(B=0), -22), (fin(Cd=0), -22),
        (fin(SH=p), -22), (fin(SH=p, pe=p, ee=p), -22), (fin(pe=p, ee=p, mi=p), -22), (fin(mi=p), -22),
        (fin(E=1 << 16, B=1 << 16, SH=p, pe=p, ee=p, mi=p), -95),
    ]
    assert [rc for rc, _ in rows] == [want for _, want in rows]


def test_predict_adaptive_rejects_bad_python_arguments():
    """ValueError before the C call, as predict_with_exit does (the engine object is built without a GPU: only the checks run)."""
    import torch
    from bayesnn_fpga_amd.engine import MCDEngine

    class Fake(MCDEngine):
        def __init__(self):            # no workspace, no device: the argument checks come first
            self.n_exits, self.chunk_samples, self.max_batch, self.out_dim, self.device = 4, 4, 8, 10, torch.device("cpu")

        def _check_x(self, x):
            return x

    e = Fake()
    x = torch.zeros(2, 3, 32, 32)
    for kw in (dict(T_max=0), dict(t_step=0), dict(t_step=5), dict(rule="entropy"), dict(test_exit=4), dict(test_exit=-5)):
        args = dict(T_max=8, threshold=0.01)
        args.update(kw)
        with pytest.raises(ValueError):
            e.predict_adaptive(x, **args)
