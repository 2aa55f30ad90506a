"""Per-pass multi-exit accuracy without a GPU: the ctypes bindings and the C ABI's host-side validation (no call reaches a kernel), the
float64 restatement ``pass_accuracy_numpy`` against torch's softmax / cumsum / topk on tie-free input, its tie rule against a stable
descending argsort, its non-finite and bad-label rules, and the assembly of the reference's metric vector from the counts against
``MultiExitAccuracy._metrics_passes``."""
import ctypes as C

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from bayesnn_fpga_amd import _lib
from bayesnn_fpga_amd.train.evaluate import (MultiExitAccuracy, exit_metric_names, exit_rows_from_counts, metric_rows_from_counts,
                                             pass_accuracy_numpy)

NEW = ("bmi_pass_accuracy_scratch_bytes", "bmi_pass_accuracy")
# (T, E, B, C, scale, seed): the issue's cases, shared with tests/test_pass_accuracy.py
CASES = [(3, 4, 37, 10, 3, 0), (2, 5, 19, 100, 4, 1), (2, 1, 8, 7, 2, 2), (2, 3, 70, 128, 5, 3), (1, 2, 5, 2, 1, 4), (4, 4, 250, 100, 3, 5)]
TOPS = (1, 5)


def make_case(T, E, B, C_, scale, seed):
    """The issue's input recipe: normal logits of the given scale, the label's logit lifted by 2 * scale with probability 0.6"""
    rng = np.random.default_rng(seed)
    l = (rng.standard_normal((T, E, B, C_)) * scale).astype(np.float32)
    y = rng.integers(0, C_, B)
    l[..., np.arange(B), y] += (rng.random((T, E, B)) < 0.6) * np.float32(2 * scale)
    return l, y


def tie_gap(l, y):
    """The tie-freeness of an input, in float64: (no other logit of a row equals the label's, the least |s_c - s_y| / max(s_c, s_y) over the
    rows and c != y of the running softmax sums)"""
    T, E, B, C_ = l.shape
    z = l.astype(np.float64)
    ex = np.exp(z - z.max(-1, keepdims=True))
    s = np.cumsum(ex / ex.sum(-1, keepdims=True), axis=1)
    other = np.arange(C_)[None, :] != y[:, None]                     # [B, C]
    ly = np.take_along_axis(l, np.broadcast_to(y[None, None, :, None], (T, E, B, 1)), -1)
    sy = np.take_along_axis(s, np.broadcast_to(y[None, None, :, None], (T, E, B, 1)), -1)
    no_equal = not ((l == ly) & other).any()
    rel = np.abs(s - sy) / np.maximum(s, sy)
    return no_equal, float(rel[np.broadcast_to(other, rel.shape)].min())


def torch_counts(l, y, tops):
    """hits [T, 2, E, K] through F.softmax, cumsum over the exits and topk (float64 on the ensemble side)"""
    lt, yt = torch.from_numpy(l), torch.from_numpy(y)
    ens = torch.cumsum(F.softmax(lt.double(), dim=-1), dim=1)
    out = []
    for score in (lt, ens):
        _, pred = score.topk(k=min(max(tops), l.shape[-1]), dim=-1)
        hit = (pred == yt[None, None, :, None]).cumsum(-1)                      # [T, E, B, k]
        out.append(torch.stack([hit[..., min(k, l.shape[-1]) - 1].sum(-1) for k in tops], dim=-1))
    return torch.stack(out, dim=1).numpy().astype(np.int32)


def test_lib_declares_the_entry_points_and_the_abi_version_stays():
    for name in NEW:
        assert name in _lib.EXPORTS
        assert hasattr(_lib.lib(), name)
    assert _lib.ABI_VERSION == 600 and _lib.lib().bmi_version() == 600
    assert _lib.PASS_ACC_MAX_TOPS == 8


def test_c_abi_validation():
    """Null pointers, counts below 1, a cut-off below 1, the three shape limits and an undersized scratch: decided on the host, before any
    launch (the device pointers are never dereferenced)."""
    lib, fake = _lib.lib(), C.c_void_p(4096)
    INVALID, UNSUPPORTED, NOMEM = -22, -95, -12
    assert lib.bmi_pass_accuracy_scratch_bytes(10, 4, 250) == 10 * 4 * 250 * 16
    assert lib.bmi_pass_accuracy_scratch_bytes(0, 4, 250) == 0 and lib.bmi_pass_accuracy_scratch_bytes(10, 4, 0) == 0
    tops = (C.c_int32 * 9)(1, 5, 2, 3, 4, 6, 7, 8, 9)
    T, E, B, Cd = 3, 4, 7, 10
    ok = [fake, T, E, B, Cd, fake, tops, 2, fake, fake, fake, fake, T * E * B * 16, None]
    for i in (0, 5, 6, 8, 9, 11):
        args = list(ok)
        args[i] = None
        assert lib.bmi_pass_accuracy(*args) == INVALID, i
    for i in (1, 2, 3, 4, 7):
        for v in (0, -1):
            args = list(ok)
            args[i] = v
            assert lib.bmi_pass_accuracy(*args) == INVALID, (i, v)
    for bad in ((0, 5), (1, 0), (1, -3)):
        args = list(ok)
        args[6] = (C.c_int32 * 2)(*bad)
        assert lib.bmi_pass_accuracy(*args) == INVALID, bad
    args = list(ok)
    args[4] = 129
    assert lib.bmi_pass_accuracy(*args) == UNSUPPORTED
    args = list(ok)
    args[2], args[12] = 33, T * 33 * B * 16
    assert lib.bmi_pass_accuracy(*args) == UNSUPPORTED
    args = list(ok)
    args[7] = 9
    assert lib.bmi_pass_accuracy(*args) == UNSUPPORTED
    args = list(ok)
    args[1], args[3], args[12] = 1 << 15, 1 << 10, (1 << 25) * E * 16            # T * B = 2^25: the grid of the first launch
    assert lib.bmi_pass_accuracy(*args) == UNSUPPORTED
    args = list(ok)
    args[12] -= 1
    assert lib.bmi_pass_accuracy(*args) == NOMEM


@pytest.mark.parametrize("case", CASES, ids=lambda c: "T{}E{}B{}C{}".format(*c[:4]))
def test_numpy_restatement_against_torch_on_tie_free_input(case):
    l, y = make_case(*case)
    no_equal, gap = tie_gap(l, y)
    print(f"{case}: least relative gap of the ensemble scores to the label's {gap:.2e}")
    assert no_equal and gap >= 1e-6               # (a condition on the input, not a measurement of the code)
    hits, maxprob, nonfinite = pass_accuracy_numpy(l, y, TOPS)
    T, E, B, C_ = l.shape
    assert hits.shape == (T, 2, E, 2) and hits.dtype == np.int32 and maxprob.shape == (T, E) and nonfinite == 0
    assert np.array_equal(hits, torch_counts(l, y, TOPS))
    rate = hits[..., 0].sum() / (T * 2 * E * B)                                  # the case's top-1 hit rate: a kernel that always or never hits fails
    print(f"{case}: top-1 hit rate {rate:.3f}")
    assert 0.17 <= rate <= 0.8, rate
    assert np.array_equal(hits[:, 1, 0], hits[:, 0, 0])                          # the ensemble of exit 0 alone is exit 0
    want = F.softmax(torch.from_numpy(l).double(), dim=-1).max(-1)[0].sum(-1).numpy()
    np.testing.assert_allclose(maxprob, want, rtol=1e-12, atol=0)


def _tied_case():
    """Small-integer logits with many duplicated values; labels at class 0, at class C - 1 and in between"""
    rng = np.random.default_rng(7)
    T, E, B, C_ = 3, 3, 24, 9
    l = rng.integers(-2, 3, (T, E, B, C_)).astype(np.float32)
    y = rng.integers(0, C_, B)
    y[:6], y[6:12] = 0, C_ - 1
    l[0, :, 12] = 1.0                              # whole rows tied
    l[1, :, 3] = 0.0
    l[1, :, 8] = -2.0
    return l, y


def test_the_tie_rule_is_a_stable_descending_sort():
    l, y = _tied_case()
    T, E, B, C_ = l.shape
    tops = (1, 2, 5, C_, C_ + 3)
    hits, _, _ = pass_accuracy_numpy(l, y, tops)
    z = l.astype(np.float64)
    ex = np.exp(z - z.max(-1, keepdims=True))
    ens = np.cumsum(ex / ex.sum(-1, keepdims=True), axis=1)
    # (equal logits give bit-equal exponentials, so the first exit's ensemble ties exactly where its logits do)
    assert ((l[:, 0, :, :, None] == l[:, 0, :, None, :]) == (ens[:, 0, :, :, None] == ens[:, 0, :, None, :])).all()
    assert (l[:, 0] == l[:, 0, :, :1]).all(-1).any()                             # there is a row whose classes all tie
    want = np.zeros_like(hits)
    for kind, score in enumerate((z, ens)):
        order = np.argsort(-score, axis=-1, kind="stable")                       # [T, E, B, C]: ties keep the lower class index first
        rank = (order == y[None, None, :, None]).argmax(-1)                      # the label's position
        want[:, kind] = (rank[..., None] < np.array(tops)).sum(2)
    assert np.array_equal(hits, want)
    assert (hits[..., 3] == B).all() and (hits[..., 4] == B).all()               # a cut-off >= C always hits
    # labels at class 0 win every tie, labels at class C - 1 lose every tie
    h0, _, _ = pass_accuracy_numpy(np.zeros((1, 1, 2, C_), np.float32), np.array([0, C_ - 1]), (1, C_ - 1, C_))
    assert h0.tolist() == [[[[1, 1, 2]], [[1, 1, 2]]]]


def test_non_finite_rows_and_bad_labels_are_misses():
    l, y = make_case(3, 4, 11, 10, 3, 9)
    base_h, base_m, nf = pass_accuracy_numpy(l, y, (1, 5, 11))
    assert nf == 0
    bad = l.copy()
    bad[0, 1, 2, 3] = np.nan
    bad[1, 0, 4, :] = np.inf
    bad[2, 3, 5, 0] = -np.inf
    yb = y.copy()
    yb[7], yb[8] = -1, 10
    h, m, nf = pass_accuracy_numpy(bad, yb, (1, 5, 11))
    assert nf == 3 and np.isfinite(m).all()
    # by hand: drop the affected (pass, exit, image) contributions from the clean result
    one_h, _, _ = pass_accuracy_numpy(l, y, (1, 5, 11))
    per = np.stack([pass_accuracy_numpy(l[:, :, b:b + 1], y[b:b + 1], (1, 5, 11))[0] for b in range(11)], axis=-1)     # [T, 2, E, K, B]
    assert np.array_equal(per.sum(-1), one_h)
    keep = np.ones((3, 2, 4, 11), dtype=bool)
    keep[0, 0, 1, 2] = False
    keep[0, 1, 1:, 2] = False                      # the ensembles from the bad exit on
    keep[1, 0, 0, 4] = False
    keep[1, 1, :, 4] = False
    keep[2, :, 3, 5] = False
    keep[..., 7] = keep[..., 8] = False            # bad labels: misses everywhere
    assert np.array_equal(h, (per * keep[:, :, :, None, :]).sum(-1))
    # the max-probability sums lose exactly the three bad rows (and keep the images with a bad label)
    zero = l.copy()
    mm = base_m.copy()
    for t, e, b in ((0, 1, 2), (1, 0, 4), (2, 3, 5)):
        z = zero[t, e].astype(np.float64)
        p = np.exp(z - z.max(-1, keepdims=True))
        mm[t, e] -= (1.0 / p.sum(-1))[b]
    np.testing.assert_allclose(m, mm, rtol=1e-12, atol=0)


@pytest.mark.parametrize("n_exits,E", [(4, 4), (1, 1), (1, 3)])
def test_metric_vector_from_counts_is_metrics_passes_bit_for_bit_on_the_top_k_entries(n_exits, E):
    """The reference's vector assembled from integer counts — float32(count) / float32(B), the CPU form of torch's fp32 mean — against the torch route on the same logits
    (CPU): every accuracy entry equal exactly, avg_maxprob within the fp32 softmax's error of the float64 one."""
    loss = MultiExitAccuracy(n_exits, acc_tops=TOPS)
    for B, seed in ((37, 0), (12, 1), (250, 2), (7, 3)):
        l, y = make_case(3, E, B, 10, 3, seed)
        assert tie_gap(l, y)[0]
        want = loss._metrics_passes(torch.from_numpy(l), torch.from_numpy(y)).numpy()          # [T, n_metrics]
        hits, maxprob, _ = pass_accuracy_numpy(l, y, TOPS)
        got = metric_rows_from_counts(loss, hits, maxprob, B, gpu_mean=False)          # (torch on the CPU divides; its GPU mean: tests/test_pass_accuracy.py)
        assert got.shape == want.shape == (3, len(loss.metric_names)) and got.dtype == np.float64
        assert np.array_equal(got[:, :-1], want[:, :-1]), (B, got - want)
        assert np.abs(got[:, -1] - want[:, -1]).max() <= 1e-6
        # grouped: a leading batch axis with its own batch size per row
        got2 = metric_rows_from_counts(loss, np.stack([hits, hits]), np.stack([maxprob, maxprob]), np.array([B, B]), gpu_mean=False)
        assert np.array_equal(got2[0], got) and np.array_equal(got2[1], got)


def test_exit_rows_from_counts_and_names():
    l, y = make_case(2, 3, 12, 10, 3, 4)
    hits, maxprob, _ = pass_accuracy_numpy(l, y, TOPS)
    rows = exit_rows_from_counts(hits, maxprob, 12)
    names = exit_metric_names(3, TOPS)
    assert rows.shape == (2, len(names)) and len(names) == 2 * 3 * 2 + 3
    assert names[:3] == ["acc1_clf0", "acc5_clf0", "acc1_clf1"] and names[6] == "acc1_ens0" and names[-1] == "maxprob2"
    assert rows[1, names.index("acc5_ens2")] == float(np.float32(hits[1, 1, 2, 1]) * (np.float32(1) / np.float32(12)))
    assert exit_rows_from_counts(hits, maxprob, 12, gpu_mean=False)[1, names.index("acc5_ens2")] == float(np.float32(hits[1, 1, 2, 1]) / np.float32(12))
    both = [exit_rows_from_counts(hits, maxprob, 8, gpu_mean=g) for g in (True, False)]
    assert np.array_equal(*both)                                                 # a power of two: the two forms agree
    assert rows[0, names.index("maxprob1")] == maxprob[0, 1] / 12
