"""CPU-side checks of the exit-ensemble read-out under row tables (bmi_forward_mcd_adaptive_ensemble, bmi_forward_mcd_exit_staged_ensemble,
bmi_finalize_ensemble_per_image and the Python keywords in front of them): every bad argument gets its answer before any launch — the
graphs live on the CPU, so a call that got as far as a launch would fail with a HIP error instead — and the contract of the two forms,
"truncate at t_used[b]" and "cut the exit sum at n_e[b]", restated in numpy on decompose_ensemble_logits."""
import ctypes as C

import numpy as np
import pytest
import torch

from bayesnn_fpga_amd import _lib
from bayesnn_fpga_amd.engine import CompiledGraph, MCDEngine, check_stop_on
from bayesnn_fpga_amd.models.resnet18.resnet18 import ResNet18MCEarlyExit
from bayesnn_fpga_amd.train.uncertainty import decompose_ensemble_logits
from tests.helpers import build_seeded, load_golden

KW = dict(dropout_exit=True, dropout="block", dropout_p=0.25, out_dim=10)


def _graph(dtype="f16", max_batch=8, chunk=4, **kw):
    return CompiledGraph(build_seeded(ResNet18MCEarlyExit, dict(KW, **kw)), "cpu", max_batch, chunk, dtype=dtype)


def test_adaptive_ensemble_entry_point_checks_arguments_before_any_launch():
    cg = _graph()
    lib, h, ws_ok, E = _lib.lib(), cg.handle, cg.workspace_bytes, cg.n_exits
    need = lib.bmi_ensemble_scratch_bytes(h, 8)
    assert need == 4 * E * 8 * 10 * 4
    buf = np.zeros(64, dtype=np.float64)                  # a non-null address; no row gets far enough to use it
    p = buf.ctypes.data
    act = (C.c_int32 * 64)()

    def ad(h=h, x=p, batch=8, t_max=8, t_step=4, rule=0, test_exit=3, stop_on=1, S1=p, SH=p, Q1=p, Q2=p, QH=p, scratch=p, sbytes=need,
           t_used=p, conv=p, nbytes=ws_ok):
        return lib.bmi_forward_mcd_adaptive_ensemble(h, x, batch, 0, t_max, t_step, 7, 0, rule, 0.01, test_exit, stop_on, S1, p, p, SH, Q1, Q2, QH,
                                                     scratch, sbytes, t_used, conv, act, p, nbytes, None)

    small = ws_ok - 1
    rows = [
        (ad(h=None), -22), (ad(Q1=None), -22), (ad(Q2=None), -22), (ad(QH=None), -22), (ad(scratch=None), -22),
        (ad(stop_on=2), -22), (ad(stop_on=-1), -22), (ad(batch=0), -22), (ad(batch=9), -22),
        (ad(sbytes=need - 1), -12), (ad(sbytes=need - 1, nbytes=small), -12), (ad(sbytes=0), -12),
        # behind the ensemble's own checks: bmi_forward_mcd_adaptive's, for both stop_on
        (ad(x=None), -22), (ad(S1=None), -22), (ad(t_used=None), -22), (ad(t_max=0), -22), (ad(t_step=0), -22), (ad(rule=2), -22),
        (ad(test_exit=E), -22), (ad(test_exit=-1), -22), (ad(t_step=5), -95), (ad(nbytes=small), -12), (ad(stop_on=0, nbytes=small), -12),
        (ad(SH=None, conv=None, nbytes=small), -12),         # the optional outputs stay optional
    ]
    assert [rc for rc, _ in rows] == [want for _, want in rows]
    assert not buf.any() and not any(act)
    exact = _graph("f32")
    need32 = lib.bmi_ensemble_scratch_bytes(exact.handle, 8)
    assert ad(h=exact.handle, sbytes=need32, nbytes=exact.workspace_bytes) == -95


def test_staged_ensemble_entry_point_checks_arguments_before_any_launch():
    cg = _graph()
    lib, h, ws_ok, E = _lib.lib(), cg.handle, cg.workspace_bytes, cg.n_exits
    need = lib.bmi_ensemble_scratch_bytes(h, 8)
    buf = np.zeros(64, dtype=np.float64)
    p = buf.ctypes.data
    act = (C.c_int32 * 64)()

    def st(h=h, batch=8, t_count=4, crit=0, ens=0, first_exit=1, S1=p, Q1=p, Q2=p, QH=p, scratch=p, sbytes=need, exit_of=p, nbytes=ws_ok):
        rule = _lib.ExitRule(crit, ens, 0.5, first_exit)
        return lib.bmi_forward_mcd_exit_staged_ensemble(h, p, batch, t_count, 7, 0, C.byref(rule), S1, p, p, p, Q1, Q2, QH, scratch, sbytes,
                                                        exit_of, act, p, nbytes, None)

    small = ws_ok - 1
    rows = [
        (st(h=None), -22), (st(Q1=None), -22), (st(Q2=None), -22), (st(QH=None), -22), (st(scratch=None), -22), (st(batch=0), -22),
        (st(batch=9), -22), (st(sbytes=need - 1), -12), (st(sbytes=need - 1, nbytes=small), -12),
        (st(S1=None), -22), (st(exit_of=None), -22), (st(crit=2), -22), (st(ens=2), -22), (st(first_exit=E), -22), (st(t_count=0), -22),
        (st(t_count=5), -95), (st(nbytes=small), -12),
    ]
    assert [rc for rc, _ in rows] == [want for _, want in rows]
    assert not buf.any() and not any(act)
    exact = _graph("f32")
    assert st(h=exact.handle, sbytes=lib.bmi_ensemble_scratch_bytes(exact.handle, 8), nbytes=exact.workspace_bytes) == -95


def test_finalize_ensemble_per_image_checks_arguments_before_any_launch():
    lib = _lib.lib()
    buf = np.zeros(64, dtype=np.float64)
    p = buf.ctypes.data

    def fin(E=4, B=8, Cd=10, t_used=p, Q1=p, Q2=p, QH=p, mean=p, var=p, pe=p, ee=p, mi=p):
        return lib.bmi_finalize_ensemble_per_image(E, B, Cd, t_used, Q1, Q2, QH, mean, var, pe, ee, mi, None, None)

    rows = [(fin(t_used=None), -22), (fin(Q1=None), -22), (fin(Q2=None), -22), (fin(QH=None), -22), (fin(mean=None), -22),
            (fin(var=None), -22), (fin(pe=None), -22), (fin(ee=None), -22), (fin(mi=None), -22), (fin(E=0), -22), (fin(B=0), -22),
            (fin(Cd=0), -22), (fin(E=1 << 16, B=1 << 16), -95)]
    assert [rc for rc, _ in rows] == [want for _, want in rows]


class _Fake(MCDEngine):
    def __init__(self):                # no workspace, no device: the argument checks come first
        self.n_exits, self.chunk_samples, self.max_batch, self.out_dim, self.device = 4, 4, 8, 10, torch.device("cpu")

    def _check_x(self, x):
        return x


def test_python_keywords_are_checked_before_the_c_call():
    assert check_stop_on("exit", False) is None and check_stop_on("exit", True) is None and check_stop_on("ensemble", True) is None
    for bad in (("ensemble", False), ("mean", True), (1, True), (None, False)):
        with pytest.raises(ValueError):
            check_stop_on(*bad)
    e = _Fake()
    x = torch.zeros(2, 3, 32, 32)
    S = torch.zeros(3, 4, 2, 10, dtype=torch.float64)
    H = torch.zeros(4, 2, dtype=torch.float64)
    Q = torch.zeros(2, 4, 2, 10, dtype=torch.float64)
    QH = torch.zeros(4, 2, dtype=torch.float64)
    with pytest.raises(ValueError, match="ensemble=True"):
        e.predict_adaptive(x, 8, 0.01, stop_on="ensemble")
    with pytest.raises(ValueError, match="stop_on"):
        e.predict_adaptive(x, 8, 0.01, ensemble=True, stop_on="both")
    bad_sums = (dict(H=None, Q=Q, QH=QH), dict(H=H, Q=None, QH=QH), dict(H=H, Q=Q, QH=None), dict(H=H, Q=Q[0], QH=QH),
                dict(H=H, Q=Q.float(), QH=QH), dict(H=H, Q=Q, QH=QH.t()), dict(H=H, Q=Q[:, :, :1], QH=QH))
    for kw in bad_sums:
        with pytest.raises(ValueError):
            e.accumulate_adaptive(x, S, 8, 0.01, ensemble=True, **kw)
    with pytest.raises(ValueError):
        e.accumulate_adaptive(x, S, 8, 0.01, H=H, Q=Q, QH=QH)              # sums of ensemble=True without it
    for kw in (dict(H=H, Q=Q), dict(H=H, QH=QH), dict(Q=Q, QH=QH), dict(H=H, Q=Q.float(), QH=QH)):
        with pytest.raises(ValueError):
            e.accumulate_early_exit(x, S, 4, 0.5, **kw)
    t_used = torch.ones(2, dtype=torch.int32)
    for args in ((Q[0], QH, t_used), (Q.float(), QH, t_used), (Q, QH[:, :1], t_used), (Q, QH, t_used.long()), (Q, QH, t_used[:1])):
        with pytest.raises(ValueError):
            e.finalize_ensemble_per_image(*args)


def rows_restatement(logits, t_used=None, n_e=None, tau=None):
    """What the row-table forms of csrc/ensemble.hip leave in (Q1, Q2, QH), in numpy: image b gets its first t_used[b] samples (None: all) and
    its first n_e[b] exits (None: all); per row the arithmetic of decompose_ensemble_logits, rows that are not computed stay zero."""
    l = np.asarray(logits, dtype=np.float32)
    T, E, B, Cn = l.shape
    if tau is not None:
        inv = (1.0 / np.asarray(tau, dtype=np.float64).astype(np.float32).astype(np.float64)).astype(np.float32)
        l = (l * inv[None, :, None, None]).astype(np.float32)
    z = l.astype(np.float64)
    z = z - z.max(-1, keepdims=True)
    p = np.exp(z) / np.exp(z).sum(-1, keepdims=True)
    Q1, Q2, QH = np.zeros((E, B, Cn)), np.zeros((E, B, Cn)), np.zeros((E, B))
    for b in range(B):
        for t in range(T if t_used is None else int(t_used[b])):
            acc = np.zeros(Cn)
            for e in range(E if n_e is None else int(n_e[b])):
                acc = acc + p[t, e, b]
                q = acc / (e + 1)
                Q1[e, b] += q
                Q2[e, b] += q * q
                with np.errstate(divide="ignore", invalid="ignore"):
                    QH[e, b] += -np.where(q > 0, q * np.log(q), 0.0).sum()
    return Q1, Q2, QH


def _readout(Q1, Q2, QH, t):
    """bmi_finalize_ensemble_per_image in numpy: t [B] per image."""
    t = np.asarray(t, dtype=np.float64)
    mean = Q1 / t[None, :, None]
    var = np.maximum(Q2 / t[None, :, None] - mean * mean, 0.0)
    with np.errstate(divide="ignore", invalid="ignore"):
        pred = -np.where(mean > 0, mean * np.log(mean), 0.0).sum(-1)
    exp = QH / t[None, :]
    return dict(mean=mean, var=var, pred_entropy=pred, exp_entropy=exp, mutual_info=np.maximum(pred - exp, 0.0))


@pytest.mark.parametrize("name", ["resnet18_block_exit", "resnet18_mask8_exit_c100", "vgg19_exit_mc"])
def test_truncation_at_t_used_is_the_fixed_run_on_the_first_samples(name):
    """Image b of the adaptive read-out = image b of decompose_ensemble_logits on the first t_used[b] passes, for any t_used: the sums are
    running sums in sample order, and dividing by the image's own count is the fixed run's division."""
    logits = np.asarray(load_golden(f"{name}.npz")["logits"])
    T, E, B, _ = logits.shape
    t_used = 1 + (np.arange(B) * 7 + 3) % T
    assert len(set(t_used.tolist())) > 1 and t_used.max() <= T
    tau = None if name.startswith("vgg") else np.linspace(0.7, 1.9, E)
    r = _readout(*rows_restatement(logits, t_used=t_used, tau=tau), t_used)
    for t in sorted(set(t_used.tolist())):
        ref = decompose_ensemble_logits(logits[:t], tau)
        at = t_used == t
        for k in ("mean", "var"):
            np.testing.assert_allclose(r[k][:, at], ref[k][:, at], rtol=0, atol=1e-15, err_msg=k)
        for k in ("pred_entropy", "exp_entropy", "mutual_info"):
            np.testing.assert_allclose(r[k][:, at], ref[k][:, at], rtol=0, atol=1e-12, err_msg=k)


@pytest.mark.parametrize("name", ["resnet18_block_exit", "resnet18_mask8_exit_c100", "vgg19_exit_mc"])
def test_cutting_the_exit_sum_at_n_e_leaves_the_reached_rows_unchanged(name):
    """Row e of the ensemble reads exits 0..e only: cut at n_e[b], rows e < n_e[b] are the full sums BIT FOR BIT and the others stay zero."""
    logits = np.asarray(load_golden(f"{name}.npz")["logits"])
    T, E, B, _ = logits.shape
    n_e = 1 + (np.arange(B) * 3 + 1) % E
    assert len(set(n_e.tolist())) > 1
    full = rows_restatement(logits)
    cut = rows_restatement(logits, n_e=n_e)
    for f, c in zip(full, cut):
        for b in range(B):
            assert np.array_equal(c[:n_e[b], b], f[:n_e[b], b]) and not c[n_e[b]:, b].any()
    ref = decompose_ensemble_logits(logits)
    r = _readout(*full, np.full(B, T))
    np.testing.assert_allclose(r["mean"], ref["mean"], rtol=0, atol=1e-15)
    np.testing.assert_allclose(r["mutual_info"], ref["mutual_info"], rtol=0, atol=1e-12)
