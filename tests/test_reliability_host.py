"""Reliability tables without a GPU: the ctypes bindings and the C ABI's host-side validation (no call reaches a kernel), the float64
restatement ``reliability_numpy`` against ``train.metrics.ece_hist_binary`` / ``nll_mse_acc`` and the golden metric vector — keys equal to
the metric's own float32 confidences first, then edges and integer bins equal exactly, ECE within the metric's float32 arithmetic, NLL and
Brier to 1e-12 —, its tie, non-finite, bad-label, equal-width, N < n_bins and zero-width-bin rules, and ``table_metrics``."""
import ctypes as C

import numpy as np
import pytest

from bayesnn_fpga_amd import _lib
from bayesnn_fpga_amd.train.metrics import ece_hist_binary, nll_mse_acc
from bayesnn_fpga_amd.train.reliability import FIX, reliability_numpy, row_names, table_metrics, width_edges
from bayesnn_fpga_amd.train.results_analyzer import exit_ensembles
from oracle import metrics as oracle_metrics
from tests.helpers import load_golden

NEW = ("bmi_reliability_record", "bmi_reliability_scratch_bytes", "bmi_reliability_table")
# (E, N, C, scale, seed, saturated share): the issue's cases, shared with tests/test_reliability.py
CASES = [(4, 250, 10, 3, 0, 0), (4, 1000, 100, 2, 1, 0.3), (2, 37, 7, 1, 2, 0), (3, 15, 10, 3, 3, 0), (2, 14, 10, 3, 4, 0), (1, 1, 5, 1, 5, 0),
         (2, 4097, 128, 4, 7, 0.5)]
# ece_hist_binary sums and averages in float32 — pairwise means of up to 2^14 values in [0, 1], 15 terms —: a worst-case bound on that
# arithmetic is about 2e-6; the restatement is exact in float64
ECE_BOUND = 2e-6
IDS = dict(ids=lambda c: "E{}N{}C{}".format(*c[:3]))


def make_case(E, N, C_, scale, seed, sat):
    """The issue's input recipe: normal logits of the given scale, the label's logit lifted by 2 * scale with probability 0.6, softmax in
    float64; the first sat * N images replaced by a one-hot on the label (p exactly 0 and 1: the clip and the duplicate key 1.0).
    -> (mean float64 [E, N, C], labels int64 [N])"""
    rng = np.random.default_rng(seed)
    l = rng.standard_normal((E, N, C_)) * scale
    y = rng.integers(0, C_, N)
    l[:, np.arange(N), y] += (rng.random((E, N)) < 0.6) * (2.0 * scale)
    ex = np.exp(l - l.max(-1, keepdims=True))
    p = ex / ex.sum(-1, keepdims=True)
    k = int(sat * N)
    if k:
        p[:, :k] = 0.0
        p[:, np.arange(k), y[:k]] = 1.0
    return p, y


def onehot(y, C_):
    o = np.zeros((len(y), C_))
    o[np.arange(len(y)), y] = 1
    return o


def metric_conf(p):
    """The float32 confidences and predictions of ece_hist_binary's own lines"""
    pc = np.clip(np.asarray(p, dtype=np.float64), 1e-256, 1 - 1e-256)
    pred = np.argmax(pc, axis=1)
    return (pc[np.arange(len(pc)), pred] / pc.sum(axis=1)).astype(np.float32), pred


def metric_table(conf, hit, n_bins=15):
    """edges, count and hits as ece_hist_binary derives them from its confidences"""
    n = len(conf)
    srt = np.sort(conf)
    edges = np.empty(n_bins + 1, dtype=np.float32)
    edges[0] = 0.0
    for i in range(n_bins):
        edges[i + 1] = srt[min((i + 1) * (n // n_bins), n - 1)]
    edges[-1] = 1.0
    sel = [(conf > lo) & (conf <= hi) for lo, hi in zip(edges[:-1], edges[1:])]
    return edges, np.array([s.sum() for s in sel]), np.array([hit[s].sum() for s in sel])


def test_lib_declares_the_entry_points_and_the_abi_version_stays():
    for name in NEW:
        assert name in _lib.EXPORTS
        assert hasattr(_lib.lib(), name)
    assert _lib.ABI_VERSION == 600 and _lib.lib().bmi_version() == 600
    assert _lib.REL_MAX_BINS == 64


def test_c_abi_validation():
    """Null pointers, counts below 1, a batch beyond the capacity, n_bins outside [1, 64], bad fixed edges, the shape limits and an
    undersized scratch: decided on the host, before any launch (the device pointers are never dereferenced)."""
    lib, fake = _lib.lib(), C.c_void_p(4096)
    INVALID, UNSUPPORTED, NOMEM = -22, -95, -12
    E, B, Cd, cap = 4, 7, 10, 20
    ok = [fake, E, B, Cd, fake, 3, cap, fake, fake, fake, fake, fake, None]
    for i in (0, 4, 7, 8, 9, 10):
        args = list(ok)
        args[i] = None
        assert lib.bmi_reliability_record(*args) == INVALID, i
    for i in (1, 2, 3, 6):
        for v in (0, -1):
            args = list(ok)
            args[i] = v
            assert lib.bmi_reliability_record(*args) == INVALID, (i, v)
    for n0, cp in ((-1, cap), (14, cap), (0, 6), (2 ** 31 - 1, 2 ** 31 - 1)):
        args = list(ok)
        args[5], args[6] = n0, cp
        assert lib.bmi_reliability_record(*args) == INVALID, (n0, cp)
    args = list(ok)
    args[3] = 129
    assert lib.bmi_reliability_record(*args) == UNSUPPORTED
    args = list(ok)
    args[1] = 33
    assert lib.bmi_reliability_record(*args) == UNSUPPORTED
    args = list(ok)
    args[2], args[5], args[6] = 1 << 25, 0, 1 << 25                             # the launch grid
    assert lib.bmi_reliability_record(*args) == UNSUPPORTED

    R, N, nb = 8, 10000, 15
    need = R * 3 * 3 * nb * 8                                                    # ceil(10000 / 4096) = 3 chunks
    assert lib.bmi_reliability_scratch_bytes(R, N, nb) == need
    assert lib.bmi_reliability_scratch_bytes(R, 4096, nb) == R * 3 * nb * 8 and lib.bmi_reliability_scratch_bytes(R, 4097, nb) == R * 2 * 3 * nb * 8
    for bad in ((0, N, nb), (R, 0, nb), (R, N, 0), (R, N, 65), (65, N, nb), (R, 1 << 22, nb)):
        assert lib.bmi_reliability_scratch_bytes(*bad) == 0, bad
    ok = [fake, fake, fake, fake, R, N, N, nb, None, fake, fake, fake, fake, fake, fake, need, None]
    for i in (0, 1, 2, 3, 9, 10, 11, 12, 13, 14):
        args = list(ok)
        args[i] = None
        assert lib.bmi_reliability_table(*args) == INVALID, i
    for i in (4, 5, 7):
        for v in (0, -1):
            args = list(ok)
            args[i] = v
            assert lib.bmi_reliability_table(*args) == INVALID, (i, v)
    args = list(ok)
    args[7] = 65
    assert lib.bmi_reliability_table(*args) == INVALID
    args = list(ok)
    args[6] = N - 1                                                              # N beyond the capacity
    assert lib.bmi_reliability_table(*args) == INVALID
    for edges in ([0.0, 0.5, 0.4, 1.0], [0.0, float("nan"), 0.5, 1.0], [0.0, 0.5, 0.6, float("inf")]):
        args = list(ok)
        args[7], args[8] = 3, (C.c_float * 4)(*edges)
        assert lib.bmi_reliability_table(*args) == INVALID, edges
    args = list(ok)
    args[4], args[15] = 65, 1 << 40
    assert lib.bmi_reliability_table(*args) == UNSUPPORTED
    args = list(ok)
    args[5], args[6], args[15] = 1 << 22, 1 << 22, 1 << 40
    assert lib.bmi_reliability_table(*args) == UNSUPPORTED
    args = list(ok)
    args[15] -= 1
    assert lib.bmi_reliability_table(*args) == NOMEM


_seen = {}


def restated(case):
    """(mean, labels, reliability_numpy of them): computed once per case"""
    if case not in _seen:
        p, y = make_case(*case)
        _seen[case] = (p, y, reliability_numpy(p, y))
    return _seen[case]


@pytest.mark.parametrize("case", CASES, **IDS)
def test_numpy_restatement_against_the_metric_functions(case):
    p, y, t = restated(case)
    E, N, C_ = p.shape
    assert t["nonfinite"] == 0 and t["badlabel"] == 0 and t["n"] == N
    assert t["keys"].shape == (2 * E, N) and t["keys"].dtype == np.uint32 and t["count"].dtype == np.int64 and t["edges"].dtype == np.float32
    rows = list(p) + list(exit_ensembles(p))
    oh = onehot(y, C_)
    m = table_metrics(t)
    # the key condition: a condition on the input (ascending against pairwise summation at a float32 rounding boundary), asserted first
    mismatches = sum(int((metric_conf(v)[0].view(np.uint32) != t["keys"][r]).sum()) for r, v in enumerate(rows))
    print(f"{case}: keys that differ from the metric's float32 confidences: {mismatches}")
    assert mismatches == 0
    worst = 0.0
    for r, v in enumerate(rows):
        conf, pred = metric_conf(v)
        hit = pred == y
        assert np.array_equal(t["hit"][r], hit.astype(np.uint8))
        edges, count, hits = metric_table(conf, hit)
        assert np.array_equal(t["edges"][r].view(np.uint32), edges.view(np.uint32))
        assert np.array_equal(t["count"][r], count) and np.array_equal(t["hits"][r], hits)
        assert t["count"][r].sum() == N                                           # every confidence is in exactly one bin
        for i in range(15):
            sel = (conf > edges[i]) & (conf <= edges[i + 1])
            assert t["conf_fix"][r, i] == int(sum(int(float(c) * FIX) for c in conf[sel]))
            assert all(float(c) * FIX == int(float(c) * FIX) for c in conf[sel][:8])     # a multiple of 2^-40
        worst = max(worst, abs(m["ece"][r] - ece_hist_binary(v, oh)))
        nll, mse, acc = nll_mse_acc(v, oh)
        np.testing.assert_allclose(m["nll"][r], nll, rtol=1e-12, atol=0)
        np.testing.assert_allclose(m["brier"][r], mse, rtol=1e-12, atol=0)
        assert m["acc"][r] == acc
    print(f"{case}: max |ece - ece_hist_binary| = {worst:.2e}")
    assert worst <= ECE_BOUND
    assert np.array_equal(t["keys"][0], t["keys"][E])                            # the ensemble of exit 0 alone is exit 0
    if case[5]:
        assert (t["keys"] == 0x3f800000).sum() >= 2 * E * int(case[5] * N)       # the duplicate key 1.0


def test_against_the_golden_metric_vector_and_the_oracle():
    """tests/golden/metrics.npz (the reference's own numbers) and oracle.metrics on its probabilities: the oracle sums a row with torch,
    so only the metrics are compared, not the keys"""
    g = load_golden("metrics.npz")
    p, oh = np.asarray(g["p"], dtype=np.float64), g["onehot"]
    m = table_metrics(reliability_numpy(p[None], oh.argmax(1)))
    assert abs(m["ece"][0] - float(g["ece_hist"])) <= ECE_BOUND and abs(m["ece"][0] - oracle_metrics.ece_hist_binary(p, oh)) <= ECE_BOUND
    nll, mse, acc = oracle_metrics.nll_mse_acc(p, oh)
    np.testing.assert_allclose([m["nll"][0], m["brier"][0]], [float(g["nll"]), float(g["mse"])], rtol=1e-12, atol=0)
    np.testing.assert_allclose([m["nll"][0], m["brier"][0]], [nll, mse], rtol=1e-12, atol=0)
    assert m["acc"][0] == float(g["acc"]) == acc
    assert np.array_equal(m["ece"][:1], m["ece"][1:])                            # one exit: its ensemble is itself


def test_the_tie_rule_is_numpy_s_argmax():
    p = np.array([[[0.25, 0.25, 0.25, 0.25], [0.1, 0.4, 0.4, 0.1], [0.0, 0.0, 0.5, 0.5]],
                  [[0.25, 0.25, 0.25, 0.25], [0.7, 0.0, 0.0, 0.3], [0.5, 0.5, 0.0, 0.0]]])
    t = reliability_numpy(p, np.array([0, 2, 2]))
    assert t["hit"].tolist() == [[1, 0, 1], [1, 0, 0], [1, 0, 1], [1, 0, 0]]     # the ensemble of image 2 ties all four classes: class 0
    assert t["keys"][0].view(np.float32).tolist() == [0.25, np.float32(0.4), 0.5]
    t = reliability_numpy(p, np.array([1, 1, 0]))
    assert t["hit"].tolist() == [[0, 1, 0], [0, 0, 1], [0, 1, 0], [0, 0, 1]]


def test_non_finite_rows_and_bad_labels():
    p, y = make_case(3, 11, 10, 3, 9, 0)
    base = reliability_numpy(p, y)
    bad, yb = p.copy(), y.copy()
    bad[1, 2, 3] = np.nan
    bad[0, 4, :] = np.inf
    bad[2, 5, 0] = -np.inf
    yb[7], yb[8] = -1, 10
    t = reliability_numpy(bad, yb)
    assert t["badlabel"] == 2 and t["nonfinite"] == (1 + 2) + (1 + 3) + (1 + 1)  # an exit's row and the ensembles from it on
    dead = np.zeros((6, 11), dtype=bool)
    dead[[1, 4, 5], 2] = dead[[0, 3, 4, 5], 4] = dead[[2, 5], 5] = True
    dead[:, 7] = dead[:, 8] = True
    for name in ("keys", "hit", "nll", "brier"):
        assert (t[name][dead] == 0).all() and np.array_equal(t[name][~dead], base[name][~dead]), name
    for name in ("edges", "count", "hits", "conf_fix", "nll_sum", "brier_sum"):
        assert np.isfinite(t[name]).all(), name
    assert np.array_equal(t["count"].sum(1), 11 - dead.sum(1))                   # key 0 falls in no bin


def test_width_binning_few_images_and_zero_width_bins():
    p, y, mass = restated(CASES[0])
    t = reliability_numpy(p, y, n_bins=10, binning="width")
    assert np.array_equal(t["edges"], np.tile(width_edges(10), (8, 1))) and t["edges"][0, 3] == np.float32(3) / np.float32(10)
    for r in range(8):
        conf = t["keys"][r].view(np.float32)
        want = [int(((conf > lo) & (conf <= hi)).sum()) for lo, hi in zip(t["edges"][r, :-1], t["edges"][r, 1:])]
        assert t["count"][r].tolist() == want and sum(want) == 250
    assert np.array_equal(t["nll_sum"].view(np.int64), mass["nll_sum"].view(np.int64))       # the sums do not depend on the bins
    with pytest.raises(ValueError):
        reliability_numpy(p, y, binning="kde")
    # N < n_bins: per = 0, every inner edge is the least confidence — bin 0 holds it, the bins between have no width
    p, y, t = restated(CASES[4])
    for r in range(4):
        least = t["keys"][r].view(np.float32).min()
        assert (t["edges"][r, 1:15] == least).all() and t["edges"][r, 0] == 0 and t["edges"][r, 15] == 1
        assert t["count"][r, 0] == (t["keys"][r].view(np.float32) == least).sum() and (t["count"][r, 1:14] == 0).all()
        assert t["count"][r].sum() == 14
    # a saturated network: many keys are exactly 1.0, the upper edges coincide and the bins between them stay empty
    p, y, t = restated(CASES[6])
    for r in range(4):
        width = np.diff(t["edges"][r])
        assert (width == 0).sum() >= 6 and (t["count"][r][width == 0] == 0).all() and t["count"][r].sum() == 4097
        assert t["count"][r][np.nonzero(width)[0][-1]] >= 2048                   # the ones sit in the last bin that has a width


def test_table_metrics_against_a_direct_computation():
    p, y, t = restated(CASES[1])
    m = table_metrics(t)
    E, N, _ = p.shape
    assert [len(m[k]) for k in ("acc", "ece", "mce", "nll", "brier")] == [2 * E] * 5
    for r in range(2 * E):
        conf = t["keys"][r].view(np.float32).astype(np.float64)
        ece, mce = 0.0, 0.0
        for i in range(15):
            sel = (conf > t["edges"][r, i]) & (conf <= t["edges"][r, i + 1])
            if sel.any():
                gap = abs(conf[sel].sum() / sel.sum() - t["hit"][r][sel].sum() / sel.sum())        # (sums of multiples of 2^-40: exact)
                ece += gap * sel.sum() / N
                mce = max(mce, gap)
        np.testing.assert_allclose([m["ece"][r], m["mce"][r]], [ece, mce], rtol=1e-13, atol=0)
        assert m["nll"][r] == t["nll_sum"][r] / N and m["brier"][r] == t["brier_sum"][r] / N and m["acc"][r] == t["hit"][r].sum() / N
    half = table_metrics(dict(t, n=2 * N))
    np.testing.assert_allclose(half["ece"], m["ece"] / 2, rtol=1e-13, atol=0)
    assert np.array_equal(table_metrics(t, n=N)["ece"], m["ece"])
    assert row_names(2) == ["0", "1", "Ensemble0", "Ensemble1"]
