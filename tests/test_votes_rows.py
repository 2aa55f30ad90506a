"""-m gpu: the image-list vote kernel and the decided-vote stop rule through their stand-alone entries (csrc/votes_rows.hip:
bmi_vote_counts_rows / bmi_vote_decide) — the counts against the numpy restatement on tests/test_votes.py's gap-checked references for
every case x calibration map x plain / weighted ensembles, rows that are not covered left alone (their logits are NaN), the null form
against bmi_vote_counts, a full launch continued by a list launch, and the rule against ``vote_decided_numpy``.  Integer equality
throughout."""
import ctypes as C

import numpy as np
import pytest
import torch

from bayesnn_fpga_amd import _lib
from bayesnn_fpga_amd.train.uncertainty import vote_counts_numpy, vote_decided_numpy
from tests.gpu_helpers import ptr, stream
from tests.test_votes import DEV, FILL, PAD, _dev, reference, run_kernel
from tests.test_votes_host import CASES, MAPS, case_id

pytestmark = pytest.mark.gpu
# the issue's cases: E = 1, E = 32 (two waves per block in the weighted form), C on both sides of 64, more than one block
ROW_CASES = [CASES[0], CASES[1], CASES[2], CASES[3], CASES[5]]
assert [c[:4] for c in ROW_CASES] == [(3, 4, 37, 10), (2, 5, 19, 100), (2, 1, 8, 7), (2, 3, 70, 128), (2, 32, 3, 65)]


def run_rows(l, weights=None, tau=None, scale=None, bias=None, matrix=None, rows=None, n_e=None, into=None, list_count=None):
    """bmi_vote_counts_rows through the C ABI on counts pre-filled with FILL (or ``into``) with canaries around them ->
    (rc, V - FILL, the counter's gain, canaries intact, the device tensor)"""
    lib = _lib.lib()
    T, E, B, C_ = l.shape
    n = 2 * E * B * C_
    ld = _dev(l)
    if into is None:
        into = torch.full((PAD + n + PAD,), -7, dtype=torch.int32, device=DEV)
        into[PAD:PAD + n] = FILL
    nf = torch.full((1,), 100, dtype=torch.int32, device=DEV)
    tau_c = None if tau is None else (C.c_float * E)(*np.asarray(tau, dtype=np.float64).tolist())
    keep = [_dev(scale), _dev(bias), _dev(matrix), _dev(weights)]
    lst = None if rows is None else _dev(np.asarray(rows, dtype=np.int32))
    ne = None if n_e is None else _dev(np.asarray(n_e, dtype=np.int32))
    cnt = (0 if rows is None else len(rows)) if list_count is None else list_count
    rc = lib.bmi_vote_counts_rows(ptr(ld), T, E, B, C_, tau_c, ptr(keep[0]), ptr(keep[1]), ptr(keep[2]), ptr(keep[3]), ptr(lst), cnt, ptr(ne),
                                  C.c_void_p(into.data_ptr() + 4 * PAD), ptr(nf), stream())
    torch.cuda.synchronize()
    v = into.cpu().numpy()
    intact = bool((v[:PAD] == -7).all() and (v[-PAD:] == -7).all())
    return rc, v[PAD:-PAD].reshape(2, E, B, C_) - FILL, int(nf.item()) - 100, intact, into


def half_list(B, seed):
    """About half the images, in order; a length that is no multiple of 4 (the last block of four waves is ragged)"""
    n = max(1, B // 2)
    if n % 4 == 0:
        n -= 1
    return np.sort(np.random.default_rng(seed).choice(B, size=n, replace=False)).astype(np.int32)


def exit_counts(E, B, seed):
    """n_e mixing 1, E and what lies between"""
    n_e = np.random.default_rng(seed).integers(1, E + 1, B).astype(np.int32)
    n_e[0] = E
    n_e[-1] = 1
    return n_e


PARAMS = [pytest.mark.parametrize("weighted", [False, True], ids=["mean", "weighted"]), pytest.mark.parametrize("kind", MAPS),
          pytest.mark.parametrize("case", ROW_CASES, ids=case_id)]


def _all(f):
    for p in PARAMS:
        f = p(f)
    return f


@_all
def test_list_and_exit_counts_cover_exactly_their_rows(case, kind, weighted):
    l, cal, W, want = reference(case, kind, weighted)
    T, E, B, C_ = l.shape
    rows = half_list(B, case[5])
    assert len(rows) % 4 and 1 <= len(rows) < B
    listed = np.zeros(B, bool)
    listed[rows] = True
    # a list: the other images' logits are NaN — never read, so never counted as bad rows
    dirty = l.copy()
    dirty[:, :, ~listed] = np.nan
    rc, V, nf, intact, _ = run_rows(dirty, weights=W, rows=rows, **cal)
    assert rc == _lib.BMI_OK and intact and nf == 0
    print(f"{case} {kind} weighted={weighted}: list of {len(rows)}: differing counts {int((V[:, :, listed] != want[:, :, listed]).sum())}")
    assert np.array_equal(V[:, :, listed], want[:, :, listed])
    assert not V[:, :, ~listed].any()                                  # still FILL
    assert np.array_equal(V, vote_counts_numpy(dirty, weights=W, rows=rows, **cal)[0])
    # exit counts: rows e >= n_e[b] are NaN and untouched, the ensembles below them are the full run's
    n_e = exit_counts(E, B, case[5])
    cut = np.arange(E)[:, None] < n_e[None, :]                         # [E, B]
    dirty = l.copy()
    dirty[:, ~cut] = np.nan
    rc, V, nf, intact, _ = run_rows(dirty, weights=W, n_e=n_e, **cal)
    assert rc == _lib.BMI_OK and intact and nf == 0
    assert np.array_equal(V[:, cut], want[:, cut]) and not V[:, ~cut].any()
    # both at once
    use = cut & listed[None, :]
    dirty = l.copy()
    dirty[:, ~use] = np.nan
    rc, V, nf, intact, _ = run_rows(dirty, weights=W, rows=rows, n_e=n_e, **cal)
    assert rc == _lib.BMI_OK and intact and nf == 0
    assert np.array_equal(V[:, use], want[:, use]) and not V[:, ~use].any()


@_all
def test_null_form_and_a_full_launch_continued_by_a_list_launch(case, kind, weighted):
    l, cal, W, want = reference(case, kind, weighted)
    T, E, B, C_ = l.shape
    # list = NULL, n_e = NULL: bmi_vote_counts, device against device
    rc, V, nf, intact, _ = run_rows(l, weights=W, **cal)
    rc0, V0, nf0, _, _ = run_kernel(l, weights=W, **cal)
    assert rc == rc0 == _lib.BMI_OK and intact and nf == nf0 == 0
    assert np.array_equal(V, V0) and np.array_equal(V, want)
    # the first part of T over every image, the rest over a list, into the same counts: adaptive sampling's sequence of launches
    h = T // 2
    rows = half_list(B, case[5] + 1)
    first, second = np.ascontiguousarray(l[:h]), l[h:].copy()
    listed = np.zeros(B, bool)
    listed[rows] = True
    second[:, :, ~listed] = np.nan
    rc, _, _, _, buf = run_rows(first, weights=W, **cal)
    rc2, V, nf, intact, _ = run_rows(second, weights=W, rows=rows, into=buf, **cal)
    assert rc == rc2 == _lib.BMI_OK and intact and nf == 0
    sums = vote_counts_numpy(first, weights=W, **cal)[0] + vote_counts_numpy(second, weights=W, rows=rows, **cal)[0]
    assert np.array_equal(V, sums)
    assert (V[:, :, listed].sum(-1) == T).all() and (V[:, :, ~listed].sum(-1) == h).all()


def test_covered_bad_rows_are_counted_and_errors_write_nothing():
    l, cal, W, want = reference(CASES[0], "none", False)
    T, E, B, C_ = l.shape
    rows = half_list(B, 3)
    bad = l.copy()
    bad[0, 1, rows[0], 2] = np.nan                                     # covered: counted, no vote from exit 1 or the ensembles from 1 on
    out = np.setdiff1d(np.arange(B), rows)
    bad[:, :, out[0]] = np.inf                                         # not covered
    rc, V, nf, intact, _ = run_rows(bad, rows=rows)
    wantb, want_nf = vote_counts_numpy(bad, rows=rows)
    assert rc == _lib.BMI_OK and intact and nf == want_nf == 1 and np.array_equal(V, wantb)
    assert V[0, 1, rows[0]].sum() == T - 1 and V[1, 0, rows[0]].sum() == T and V[1, E - 1, rows[0]].sum() == T - 1
    for cnt in (0, -1, B + 1):
        rc, V, nf, intact, _ = run_rows(l, rows=rows, list_count=cnt)
        assert rc == -22 and intact and nf == 0 and not V.any(), cnt
    rc, V, nf, intact, _ = run_rows(l, rows=rows, tau=[1.0, 0.0, 1.0, 1.0])
    assert rc == -22 and intact and nf == 0 and not V.any()


def run_decide(V, kind, test_exit, t, t_max, slack, active=None):
    """bmi_vote_decide through the C ABI -> (rc, the out-list, t_used with -1 where nothing was written)"""
    lib = _lib.lib()
    _, E, B, C_ = V.shape
    Vd = _dev(V.astype(np.int32))
    lst = None if active is None else _dev(np.asarray(active, dtype=np.int32))
    n = B if active is None else len(active)
    out = torch.full((PAD + n + PAD,), -7, dtype=torch.int32, device=DEV)
    count = torch.full((1,), -7, dtype=torch.int32, device=DEV)
    t_used = torch.full((B,), -1, dtype=torch.int32, device=DEV)
    rc = lib.bmi_vote_decide(ptr(Vd), E, B, C_, kind, test_exit, t, t_max, slack, ptr(lst), n, C.c_void_p(out.data_ptr() + 4 * PAD), ptr(count),
                             ptr(t_used), stream())
    torch.cuda.synchronize()
    o, k = out.cpu().numpy(), int(count.item())
    assert (o[:PAD] == -7).all() and (o[-PAD:] == -7).all()
    if rc == _lib.BMI_OK:
        assert 0 <= k <= n and (o[PAD + k:PAD + n] == -7).all()        # nothing behind the survivors
    return rc, o[PAD:PAD + max(k, 0)], t_used.cpu().numpy()


def check_decide(V, kind, test_exit, t, t_max, slack, active=None):
    B = V.shape[2]
    imgs = np.arange(B) if active is None else np.asarray(active)
    decided, _ = vote_decided_numpy(V[kind, test_exit], t, t_max, slack)
    rc, out, t_used = run_decide(V, kind, test_exit, t, t_max, slack, active)
    assert rc == _lib.BMI_OK
    assert out.tolist() == [int(b) for b in imgs if not decided[b]]    # the survivors, in the list's order
    want_t = np.full(B, -1)
    want_t[imgs] = t
    assert np.array_equal(t_used, want_t)
    return decided


def test_decide_on_constructed_counts():
    rows = [[5, 5, 0, 0], [5, 0, 0, 5], [2, 6, 3, 0], [3, 6, 2, 0], [0, 0, 0, 0], [0, 0, 10, 0], [1, 2, 3, 4], [0, 4, 0, 6]]
    V = np.zeros((2, 2, len(rows), 4), np.int32)
    V[1, 1] = rows                                                     # the other three blocks stay zero: reading the wrong one shows
    d = check_decide(V, 1, 1, 10, 16, 0)
    assert d.tolist() == [False, False, False, False, False, True, False, False]
    assert check_decide(V, 1, 1, 10, 16, 3).tolist() == [False, False, True, False, False, True, False, False]
    assert check_decide(V, 1, 1, 10, 16, 4).tolist() == [False, False, True, True, False, True, False, False]
    assert check_decide(V, 1, 1, 10, 16, 6).all() and check_decide(V, 1, 1, 10, 16, 1000).all()        # slack >= T_max - t
    assert check_decide(V, 1, 1, 16, 16, 0).all()                      # r = 0 at T_max
    assert not check_decide(V, 0, 1, 10, 16, 0).any() and not check_decide(V, 1, 0, 10, 16, 0).any()   # all-zero blocks
    check_decide(V, 1, 1, 10, 16, 3, active=[6, 2, 0, 5, 3])           # a list, not ascending: its order is kept
    # C = 1: nothing to be overtaken by
    V1 = np.zeros((2, 1, 3, 1), np.int32)
    V1[0, 0, :, 0] = [0, 1, 4]
    assert check_decide(V1, 0, 0, 4, 16, 0).all()
    # more images than one round of waves, C beyond one pass of the lanes, a list with a ragged last round
    rng = np.random.default_rng(5)
    Vr = np.zeros((2, 3, 70, 100), np.int32)
    for b in range(70):
        np.add.at(Vr[0, 2, b], rng.choice(100, size=12, p=None if b % 3 else np.r_[0.9, np.full(99, 0.1 / 99)]), 1)
    d = check_decide(Vr, 0, 2, 12, 16, 0)
    assert d.any() and not d.all()
    check_decide(Vr, 0, 2, 12, 16, 2, active=np.sort(rng.choice(70, size=37, replace=False)))
    # errors: decided on the host, nothing written
    for kw in (dict(kind=2), dict(test_exit=3), dict(t=0), dict(t=17), dict(slack=-1)):
        args = dict(kind=0, test_exit=2, t=12, t_max=16, slack=0)
        args.update(kw)
        rc, out, t_used = run_decide(Vr, **args)
        assert rc == -22 and len(out) == 0 and (t_used == -1).all(), kw
