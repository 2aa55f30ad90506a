"""Votes under adaptive sampling and staged exit, without a GPU: the ctypes bindings and the C ABI's host-side validation of the four new
entry points (no call reaches a kernel), the Python keyword checks, the image-list form of ``vote_counts_numpy`` against the full form,
and ``vote_decided_numpy`` against a brute-force enumeration of every way the remaining passes can vote."""
import ctypes as C
import itertools

import numpy as np
import pytest
import torch

from bayesnn_fpga_amd import _lib
from bayesnn_fpga_amd.engine import CompiledGraph, MCDEngine
from bayesnn_fpga_amd.models.resnet18.resnet18 import ResNet18MCEarlyExit
from bayesnn_fpga_amd.train.uncertainty import vote_counts_numpy, vote_decided_numpy
from tests.helpers import build_seeded
from tests.test_pass_accuracy_host import make_case
from tests.test_votes_host import CASES, MAPS, make_map, make_weights

NEW = ("bmi_vote_counts_rows", "bmi_vote_decide", "bmi_forward_mcd_adaptive_votes", "bmi_forward_mcd_exit_staged_votes")
KW = dict(dropout_exit=True, dropout="block", dropout_p=0.25, out_dim=10)
INVALID, NOMEM, UNSUPPORTED = -22, -12, -95


def test_lib_declares_the_entry_points_and_the_abi_version_stays():
    for name in NEW:
        assert name in _lib.EXPORTS
        assert hasattr(_lib.lib(), name)
    assert _lib.ABI_VERSION == 600 and _lib.lib().bmi_version() == 600
    assert _lib.VOTE_STOP_RULES == {"sem": 0, "margin": 1, "votes": 2} and _lib.STOP_RULES == {"sem": 0, "margin": 1}


def test_stand_alone_entries_validate_on_the_host():
    """bmi_vote_counts_rows and bmi_vote_decide on fake device pointers: every answer is decided before a launch."""
    lib, fake, other = _lib.lib(), C.c_void_p(4096), C.c_void_p(8192)
    T, E, B, Cd = 3, 4, 7, 10
    tau = (C.c_float * 33)(*([1.5] * 33))
    # bmi_vote_counts_rows(logits, T, E, B, C, tau, scale, bias, matrix, W, list, list_count, n_e, V, nonfinite, stream)
    ok = [fake, T, E, B, Cd, None, None, None, None, None, fake, 3, fake, fake, None, None]
    for i in (0, 13):
        args = list(ok)
        args[i] = None
        assert lib.bmi_vote_counts_rows(*args) == INVALID, i
    for i in (1, 2, 3, 4):
        for v in (0, -1):
            args = list(ok)
            args[i] = v
            assert lib.bmi_vote_counts_rows(*args) == INVALID, (i, v)
    for n in (0, -1, B + 1):
        args = list(ok)
        args[11] = n
        assert lib.bmi_vote_counts_rows(*args) == INVALID, n
    for maps in (dict(tau=tau, scale=fake, bias=fake), dict(scale=fake, matrix=fake, bias=fake), dict(bias=fake), dict(scale=fake)):
        args = list(ok)
        args[5], args[6], args[7], args[8] = maps.get("tau"), maps.get("scale"), maps.get("bias"), maps.get("matrix")
        assert lib.bmi_vote_counts_rows(*args) == INVALID, sorted(maps)
    args = list(ok)
    args[5] = (C.c_float * E)(1.0, 0.0, 1.0, 1.0)
    assert lib.bmi_vote_counts_rows(*args) == INVALID
    args = list(ok)
    args[4] = 129
    assert lib.bmi_vote_counts_rows(*args) == UNSUPPORTED
    args = list(ok)
    args[2], args[5] = 33, tau
    assert lib.bmi_vote_counts_rows(*args) == UNSUPPORTED
    # bmi_vote_decide(V, E, B, C, kind, test_exit, t, t_max, slack, in_list, in_count, out_list, count, t_used, stream)
    ok = [fake, E, B, Cd, 1, 2, 4, 16, 0, other, 3, fake, fake, fake, None]
    for i in (0, 11, 12, 13):
        args = list(ok)
        args[i] = None
        assert lib.bmi_vote_decide(*args) == INVALID, i
    for i, v in ((1, 0), (2, 0), (3, 0), (4, -1), (4, 2), (5, -1), (5, E), (6, 0), (7, 3), (8, -1), (10, 0), (10, B + 1)):
        args = list(ok)
        args[i] = v
        assert lib.bmi_vote_decide(*args) == INVALID, (i, v)
    args = list(ok)
    args[9] = fake                                                     # out_list == in_list
    assert lib.bmi_vote_decide(*args) == INVALID
    # the forward entries: a null handle, before anything else
    assert lib.bmi_forward_mcd_adaptive_votes(None, fake, 1, 0, 4, 2, 0, 0, 2, 0.0, 0, 0, *([fake] * 10), 1 << 20, fake, fake,
                                              (C.c_int32 * 4)(), fake, 1 << 20, None) == INVALID
    rule = _lib.ExitRule(0, 0, 0.5, 0)
    assert lib.bmi_forward_mcd_exit_staged_votes(None, fake, 1, 4, 0, 0, C.byref(rule), *([fake] * 10), 1 << 20, fake, (C.c_int32 * 4)(), fake,
                                                 1 << 20, None) == INVALID


def test_forward_entries_check_arguments_before_any_launch():
    """The two forward entries on a graph that lives on the CPU (a call that got as far as a launch would fail with a HIP error instead);
    the older adaptive entries keep refusing rule 2; nothing is written."""
    cg = CompiledGraph(build_seeded(ResNet18MCEarlyExit, KW), "cpu", 8, 4, dtype="f16")
    lib, h, ws_ok, E = _lib.lib(), cg.handle, cg.workspace_bytes, cg.n_exits
    need = lib.bmi_ensemble_scratch_bytes(h, 8)
    buf = np.zeros(64, dtype=np.float64)                  # a non-null address; no row gets far enough to use it
    p = buf.ctypes.data
    act = (C.c_int32 * 64)()
    small = ws_ok - 1

    def av(h=h, x=p, batch=8, t_max=8, t_step=4, rule=2, thr=0.0, test_exit=3, stop_on=1, S1=p, SH=p, Q1=p, QH=p, V=p, nf=p, scratch=p,
           sbytes=need, t_used=p, conv=p, nbytes=ws_ok):
        return lib.bmi_forward_mcd_adaptive_votes(h, x, batch, 0, t_max, t_step, 7, 0, rule, thr, test_exit, stop_on, S1, p, p, SH, Q1, p, QH, V, nf,
                                                  scratch, sbytes, t_used, conv, act, p, nbytes, None)

    rows = [
        (av(h=None), INVALID), (av(V=None), INVALID), (av(Q1=None), INVALID), (av(QH=None), INVALID), (av(scratch=None), INVALID),
        (av(stop_on=2), INVALID), (av(stop_on=-1), INVALID), (av(batch=0), INVALID), (av(batch=9), INVALID),
        (av(sbytes=need - 1), NOMEM), (av(sbytes=0), NOMEM), (av(sbytes=need - 1, nbytes=small), NOMEM),
        (av(thr=0.5), INVALID), (av(thr=-1.0), INVALID), (av(thr=float("nan")), INVALID), (av(thr=float("inf")), INVALID),
        (av(thr=0.5, nbytes=small), INVALID), (av(rule=3), INVALID), (av(rule=3, nbytes=small), INVALID), (av(rule=-1), INVALID),
        (av(x=None), INVALID), (av(S1=None), INVALID), (av(t_used=None), INVALID), (av(t_max=0), INVALID), (av(t_step=0), INVALID),
        (av(test_exit=E), INVALID), (av(test_exit=-1), INVALID), (av(t_step=5), UNSUPPORTED),
        # everything in order but the workspace: rule 2 with a whole slack, the moment rules with any threshold, the optional outputs
        (av(nbytes=small), NOMEM), (av(thr=3.0, stop_on=0, nbytes=small), NOMEM), (av(rule=0, thr=0.01, nbytes=small), NOMEM),
        (av(rule=1, thr=2.5, nbytes=small), NOMEM), (av(SH=None, conv=None, nf=None, nbytes=small), NOMEM),
    ]
    assert [rc for rc, _ in rows] == [want for _, want in rows]

    # the entries that were there keep answering BMI_ERR_INVALID to rule 2
    assert lib.bmi_forward_mcd_adaptive(h, p, 8, 0, 8, 4, 7, 0, 2, 0.0, 3, p, p, p, p, p, p, act, p, ws_ok, None) == INVALID
    assert lib.bmi_forward_mcd_adaptive_ensemble(h, p, 8, 0, 8, 4, 7, 0, 2, 0.0, 3, 1, p, p, p, p, p, p, p, p, need, p, p, act, p, ws_ok,
                                                 None) == INVALID

    def sv(h=h, batch=8, t_count=4, crit=0, first_exit=1, S1=p, Q1=p, V=p, nf=p, scratch=p, sbytes=need, exit_of=p, nbytes=ws_ok):
        rule = _lib.ExitRule(crit, 0, 0.5, first_exit)
        return lib.bmi_forward_mcd_exit_staged_votes(h, p, batch, t_count, 7, 0, C.byref(rule), S1, p, p, p, Q1, p, p, V, nf, scratch, sbytes,
                                                     exit_of, act, p, nbytes, None)

    rows = [
        (sv(h=None), INVALID), (sv(V=None), INVALID), (sv(Q1=None), INVALID), (sv(scratch=None), INVALID), (sv(batch=0), INVALID),
        (sv(batch=9), INVALID), (sv(sbytes=need - 1), NOMEM), (sv(sbytes=need - 1, nbytes=small), NOMEM), (sv(S1=None), INVALID),
        (sv(exit_of=None), INVALID), (sv(crit=2), INVALID), (sv(first_exit=E), INVALID), (sv(t_count=0), INVALID), (sv(t_count=5), UNSUPPORTED),
        (sv(nbytes=small), NOMEM), (sv(nf=None, nbytes=small), NOMEM),
    ]
    assert [rc for rc, _ in rows] == [want for _, want in rows]
    assert not buf.any() and not any(act)


def test_the_exact_engine_is_refused():
    cg = CompiledGraph(build_seeded(ResNet18MCEarlyExit, KW), "cpu", 8, 4, dtype="f32")
    lib, h = _lib.lib(), cg.handle
    need = lib.bmi_ensemble_scratch_bytes(h, 8)
    buf = np.zeros(64, dtype=np.float64)
    p = buf.ctypes.data
    act = (C.c_int32 * 8)()
    rc = lib.bmi_forward_mcd_adaptive_votes(h, p, 8, 0, 8, 4, 7, 0, 2, 0.0, 3, 0, p, p, p, p, p, p, p, p, p, p, need, p, p, act, p, cg.workspace_bytes,
                                            None)
    assert rc == UNSUPPORTED and not buf.any()


def test_python_keyword_checks():
    """ValueError before the C call (the engine object is built without a GPU: only the checks run)."""

    class Fake(MCDEngine):
        def __init__(self):
            self.n_exits, self.chunk_samples, self.max_batch, self.out_dim, self.device = 4, 4, 8, 10, torch.device("cpu")

        def _check_x(self, x):
            return x

    e = Fake()
    x = torch.zeros(2, 3, 32, 32)
    S, H = torch.zeros(3, 4, 2, 10, dtype=torch.float64), torch.zeros(4, 2, dtype=torch.float64)
    Q, QH = torch.zeros(2, 4, 2, 10, dtype=torch.float64), torch.zeros(4, 2, dtype=torch.float64)
    V = torch.zeros(2, 4, 2, 10, dtype=torch.int32)
    with pytest.raises(ValueError, match="ensemble=True"):                     # V without ensemble
        e.accumulate_adaptive(x, S, 8, 0.01, H=H, V=V)
    with pytest.raises(ValueError, match="needs V"):                           # rule="votes" without V
        e.accumulate_adaptive(x, S, 8, 0, rule="votes", H=H, ensemble=True, Q=Q, QH=QH)
    with pytest.raises(ValueError, match="rule must be one of"):
        e.predict_adaptive(x, 8, 0, rule="votes", ensemble=True)
    for slack in (0.5, -1, float("nan")):                                      # a slack that is no whole number >= 0
        with pytest.raises(ValueError, match="slack"):
            e.accumulate_adaptive(x, S, 8, slack, rule="votes", H=H, ensemble=True, Q=Q, QH=QH, V=V)
    with pytest.raises(ValueError, match="rule must be one of"):
        e.accumulate_adaptive(x, S, 8, 0, rule="entropy", H=H, ensemble=True, Q=Q, QH=QH, V=V)
    with pytest.raises(ValueError, match="ensemble=True"):
        e.predict_adaptive(x, 8, 0.01, votes=True)
    with pytest.raises(ValueError, match="ensemble_readout=True"):
        e.predict_early_exit(x, 4, 0.5, votes=True)
    with pytest.raises(ValueError, match="Q / QH"):                            # V without the ensemble sums
        e.accumulate_early_exit(x, S, 4, 0.5, H=H, V=V)


@pytest.mark.parametrize("weighted", [False, True], ids=["mean", "weighted"])
@pytest.mark.parametrize("kind", MAPS)
@pytest.mark.parametrize("case", [CASES[0], CASES[2], CASES[5]], ids=lambda c: "T{}E{}B{}C{}".format(*c[:4]))
def test_rows_form_of_the_restatement(case, kind, weighted):
    """rows= / n_e= give the full restatement's counts on the rows they cover and zero elsewhere; NaN logits outside count for nothing."""
    l, _ = make_case(*case)
    T, E, B, C_ = l.shape
    cal = make_map(kind, E, C_, case[5])
    W = make_weights(E, case[5]) if weighted else None
    full, _ = vote_counts_numpy(l, weights=W, **cal)
    rng = np.random.default_rng(case[5])
    rows = np.sort(rng.choice(B, size=max(1, B // 2), replace=False))
    n_e = rng.integers(1, E + 1, B)
    use = np.zeros((E, B), bool)
    use[:, rows] = True
    use &= np.arange(E)[:, None] < n_e[None, :]
    dirty = l.copy()
    dirty[:, ~use] = np.nan
    V, nf = vote_counts_numpy(dirty, weights=W, rows=rows, n_e=n_e, **cal)
    assert nf == 0 and V.dtype == np.int32
    assert np.array_equal(V[:, use], full[:, use]) and not V[:, ~use].any()
    # each of the two alone, and neither
    V1, _ = vote_counts_numpy(l, weights=W, rows=rows, **cal)
    assert np.array_equal(V1[:, :, rows], full[:, :, rows]) and V1.sum() == full[:, :, rows].sum()
    V2, _ = vote_counts_numpy(l, weights=W, n_e=n_e, **cal)
    cut = np.arange(E)[:, None] < n_e[None, :]
    assert np.array_equal(V2[:, cut], full[:, cut]) and not V2[:, ~cut].any()
    assert np.array_equal(vote_counts_numpy(l, weights=W, rows=np.arange(B), n_e=np.full(B, E), **cal)[0], full)
    # a bad row that IS covered counts, one that is not does not
    bad = l.copy()
    b_in, b_out = int(rows[0]), int(np.setdiff1d(np.arange(B), rows)[0]) if len(rows) < B else None
    bad[0, 0, b_in, 0] = np.inf
    if b_out is not None:
        bad[0, 0, b_out, 0] = np.nan
    assert vote_counts_numpy(bad, weights=W, rows=rows, **cal)[1] == 1


def _brute_force_decided(v, r):
    """Whether the lowest arg-max of counts v is the same after EVERY way r further passes can vote (each pass: one class, or none)"""
    c1 = int(np.argmax(v))
    C_ = len(v)
    for extra in itertools.product(range(C_ + 1), repeat=r):           # C_ = "this pass casts no vote"
        w = np.array(v)
        for k in extra:
            if k < C_:
                w[k] += 1
        if int(np.argmax(w)) != c1:
            return False
    return True


@pytest.mark.parametrize("C_", [1, 2, 3, 4])
def test_decided_rule_against_brute_force(C_):
    """Every count vector with t <= T_max <= 6 votes, C <= 4: decided(slack = 0) iff no completion of the remaining passes changes the lowest
    arg-max — the theorem and its converse, the lower-index tie term and C = 1 included."""
    seen = {True: 0, False: 0}
    for T_max in range(1, 7 if C_ < 4 else 6):
        for v in itertools.product(range(T_max + 1), repeat=C_):
            t = sum(v)
            if not 1 <= t <= T_max:
                continue
            decided, lead = vote_decided_numpy(np.array(v), t, T_max)
            want = _brute_force_decided(v, T_max - t)
            assert bool(decided) == want, (v, T_max, int(lead))
            seen[want] += 1
            if C_ == 1:
                assert lead == np.iinfo(np.int32).max
    assert seen[True] and (C_ == 1 or seen[False])


def test_decided_rule_by_hand():
    V = np.array([[5, 5, 0], [5, 0, 5], [2, 6, 3], [3, 6, 2], [0, 0, 0], [0, 0, 9]])
    decided, lead = vote_decided_numpy(V, 10, 16)
    assert lead.tolist() == [0, 0, 3, 2, 0, 8]             # a tie at the top: 0; runner-up above c1: the gap; below c1: the gap less 1
    assert decided.tolist() == [False, False, False, False, False, True]
    assert vote_decided_numpy(V, 10, 16, slack=3)[0].tolist() == [False, False, True, False, False, True]
    assert vote_decided_numpy(V, 10, 16, slack=6)[0].all() and vote_decided_numpy(V, 10, 16, slack=100)[0].all()
    assert vote_decided_numpy(V, 16, 16)[0].all()          # r = 0 at T_max: every image
    d, l1 = vote_decided_numpy(np.array([[4]]), 4, 16)
    assert d.all() and l1[0] == np.iinfo(np.int32).max
