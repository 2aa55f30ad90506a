"""Classwise reliability tables without a GPU: the ctypes bindings and the C ABI's host-side validation (no call reaches a kernel), the
restatement ``classwise_numpy`` against a per-class float64 histogram written here from ``p / p.sum`` by explicit comparisons (keys first:
the condition; then counts, hits, mass edges and the truncated fixed-point sums exactly), its relation to the top-label records, its zero,
one, flush, threshold, non-finite and bad-label rules, ``classwise_metrics`` against a direct classwise ECE, and a table worked by hand."""
import ctypes as C

import numpy as np
import pytest

from bayesnn_fpga_amd import _lib
from bayesnn_fpga_amd.train.reliability import FIX, classwise_metrics, classwise_numpy, reliability_numpy
from tests.test_reliability_host import make_case

NEW = ("bmi_classwise_record", "bmi_classwise_table")
# (E, N, C, scale, seed, saturated share): the issue's cases, shared with tests/test_classwise.py
CASES = [(1, 1, 1, 1, 5, 0), (2, 37, 7, 1, 2, 0), (3, 15, 10, 3, 3, 0), (2, 14, 10, 3, 4, 0), (4, 250, 100, 2, 1, 0.3),
         (2, 4097, 128, 4, 7, 0.5)]
IDS = dict(ids=lambda c: "E{}N{}C{}".format(*c[:3]))
BINS = (1, 10, 15, 64)
INVALID = 0xFFFFFFFF
ONE = 0x3F800000
THRESHOLD_EDGES = [0.01, 0.1, 0.25, 0.5, 0.75, 1.0]      # the fixed edges with edges[0] = 0.01, shared with tests/test_classwise.py


def test_lib_declares_the_entry_points_and_the_abi_version_stays():
    for name in NEW:
        assert name in _lib.EXPORTS
        assert hasattr(_lib.lib(), name)
    assert _lib.ABI_VERSION == 600 and _lib.lib().bmi_version() == 600


def test_c_abi_validation():
    """Null pointers, counts below 1, a batch beyond the capacity, n_bins outside [1, 64], bad fixed edges and the shape limits: decided on
    the host, before any launch (the device pointers are fakes and never dereferenced)."""
    lib, fake = _lib.lib(), C.c_void_p(4096)
    INVALID_, UNSUPPORTED = -22, -95
    E, B, Cd, cap = 4, 7, 10, 20
    ok = [fake, E, B, Cd, fake, 3, cap, fake, fake, fake, None]
    for i in (0, 4, 7, 8):
        args = list(ok)
        args[i] = None
        assert lib.bmi_classwise_record(*args) == INVALID_, i
    for i in (1, 2, 3, 6):
        for v in (0, -1):
            args = list(ok)
            args[i] = v
            assert lib.bmi_classwise_record(*args) == INVALID_, (i, v)
    for n0, cp in ((-1, cap), (14, cap), (0, 6), (2 ** 31 - 1, 2 ** 31 - 1)):
        args = list(ok)
        args[5], args[6] = n0, cp
        assert lib.bmi_classwise_record(*args) == INVALID_, (n0, cp)
    for i, v in ((3, 129), (1, 33)):
        args = list(ok)
        args[i] = v
        assert lib.bmi_classwise_record(*args) == UNSUPPORTED, (i, v)
    args = list(ok)
    args[2], args[5], args[6] = 1 << 25, 0, 1 << 25                             # the launch grid
    assert lib.bmi_classwise_record(*args) == UNSUPPORTED

    R, N, nb = 8, 10000, 15
    ok = [fake, fake, R, Cd, N, N, nb, None, fake, fake, fake, fake, fake, None]
    for i in (0, 1, 8, 9, 10, 11, 12):
        args = list(ok)
        args[i] = None
        assert lib.bmi_classwise_table(*args) == INVALID_, i
    for i in (2, 3, 4, 6):
        for v in (0, -1):
            args = list(ok)
            args[i] = v
            assert lib.bmi_classwise_table(*args) == INVALID_, (i, v)
    args = list(ok)
    args[6] = 65
    assert lib.bmi_classwise_table(*args) == INVALID_
    args = list(ok)
    args[5] = N - 1                                                              # N beyond the capacity
    assert lib.bmi_classwise_table(*args) == INVALID_
    for edges in ([0.0, 0.5, 0.4, 1.0], [0.0, float("nan"), 0.5, 1.0], [0.0, 0.5, 0.6, float("inf")]):
        args = list(ok)
        args[6], args[7] = 3, (C.c_float * 4)(*edges)
        assert lib.bmi_classwise_table(*args) == INVALID_, edges
    for i, v in ((2, 65), (3, 129)):
        args = list(ok)
        args[i] = v
        assert lib.bmi_classwise_table(*args) == UNSUPPORTED, (i, v)
    args = list(ok)
    args[4], args[5] = 1 << 22, 1 << 22
    assert lib.bmi_classwise_table(*args) == UNSUPPORTED


_seen = {}


def restated(case, n_bins=15, binning="width", edges=None):
    """(mean, labels, classwise_numpy of them): computed once per (case, bins)"""
    key = (case, n_bins, binning, None if edges is None else tuple(edges))
    if key not in _seen:
        if case not in _seen:
            _seen[case] = make_case(*case)
        p, y = _seen[case]
        _seen[key] = (p, y, classwise_numpy(p, y, n_bins, binning, edges))
    return _seen[key]


def direct_conf(p):
    """float32 [R, C, N]: p / p.sum of the exits and of the exit ensembles, zero below 2^-126 — numpy's own sums, not the restatement's"""
    E = p.shape[0]
    rows = np.concatenate([p, np.cumsum(p, axis=0) / np.arange(1, E + 1, dtype=np.float64)[:, None, None]])
    pc = np.clip(rows, 1e-256, None)
    q = pc / pc.sum(axis=2, keepdims=True)
    return np.where(q < 2.0 ** -126, 0.0, q).astype(np.float32).transpose(0, 2, 1).copy()


_fix = {}


def python_fix(case, conf):
    """int64 [R, C, N]: int(float(conf) * 2**40) of every confidence, formed one by one with Python integers"""
    if case not in _fix:
        _fix[case] = np.array([int(float(v) * 2 ** 40) for v in conf.reshape(-1).tolist()], dtype=np.int64).reshape(conf.shape)
    return _fix[case]


def direct_table(conf, y, edges, fix):
    """count, hits, conf_fix [R, C, n_bins] by explicit float64 comparisons against edges [R, C, n_bins + 1]"""
    R, Cd, N = conf.shape
    n_bins = edges.shape[-1] - 1
    c64, e64 = conf.astype(np.float64), edges.astype(np.float64)
    mine = y[None, None, :] == np.arange(Cd)[None, :, None]
    out = np.zeros((3, R, Cd, n_bins), dtype=np.int64)
    for i in range(n_bins):
        above = c64 >= e64[..., :1] if i == 0 else c64 > e64[..., i:i + 1]
        sel = above & (c64 <= e64[..., i + 1:i + 2])
        out[0, ..., i] = sel.sum(-1)
        out[1, ..., i] = (sel & mine).sum(-1)
        out[2, ..., i] = (fix * sel).sum(-1)                # (int64 sums of integers below 2^41: exact)
    return out


@pytest.mark.parametrize("case", CASES, **IDS)
def test_numpy_restatement_against_a_direct_histogram(case):
    p, y = restated(case)[:2]
    E, N, Cd = p.shape
    conf = direct_conf(p)
    fix = python_fix(case, conf)
    keys = conf.view(np.uint32)
    rank_sorted = np.sort(keys, axis=-1)
    for binning in ("width", "mass"):
        for n_bins in BINS:
            t = restated(case, n_bins, binning)[2]
            assert t["pkeys"].shape == (2 * E, Cd, N) and t["pkeys"].dtype == np.uint32 and t["edges"].dtype == np.float32
            assert t["count"].dtype == np.int64 and t["count"].shape == (2 * E, Cd, n_bins) and t["n"] == N
            assert t["nonfinite"] == 0 and t["badlabel"] == 0 and (t["valid"] == N).all() and np.array_equal(t["labels"], y)
            # the key condition: a condition on the input (ascending against pairwise summation at a float32 rounding boundary), asserted first
            mismatches = int((keys != t["pkeys"]).sum())
            if (binning, n_bins) == ("width", 1):
                print(f"{case}: keys that differ from p / p.sum in float32: {mismatches} of {keys.size}")
            assert mismatches == 0
            if binning == "mass":
                edges = np.empty((2 * E, Cd, n_bins + 1), dtype=np.float32)
                edges[..., 0] = 0.0
                for i in range(n_bins):
                    edges[..., i + 1] = rank_sorted[..., min((i + 1) * (N // n_bins), N - 1)].view(np.float32)
                edges[..., n_bins] = 1.0
            else:
                edges = np.broadcast_to(np.array([np.float32(i) / np.float32(n_bins) for i in range(n_bins + 1)], dtype=np.float32),
                                        (2 * E, Cd, n_bins + 1))
            assert np.array_equal(t["edges"].view(np.uint32), np.ascontiguousarray(edges).view(np.uint32)), (binning, n_bins)
            count, hits, conf_fix = direct_table(conf, y, edges, fix)
            assert np.array_equal(t["count"], count) and np.array_equal(t["hits"], hits), (binning, n_bins)
            assert np.array_equal(t["conf_fix"], conf_fix), (binning, n_bins)
            assert (t["count"].sum(-1) == N).all()                               # edges from 0 to 1: every pair is in exactly one bin
    if N * Cd <= 4000:                                                           # the sum itself with Python integers
        t = restated(case, 15, "width")[2]
        for r in range(2 * E):
            for c in range(Cd):
                for i in range(15):
                    lo, hi = float(t["edges"][r, c, i]), float(t["edges"][r, c, i + 1])
                    vals = [float(v) for v in conf[r, c] if (v >= lo if i == 0 else v > lo) and v <= hi]
                    assert int(t["conf_fix"][r, c, i]) == sum(int(v * 2 ** 40) for v in vals)
    assert np.array_equal(t["pkeys"][0], t["pkeys"][E])                          # the ensemble of exit 0 alone is exit 0


@pytest.mark.parametrize("case", CASES, **IDS)
def test_relation_to_the_top_label_records(case):
    p, y, t = restated(case)
    top = reliability_numpy(p, y)
    E, N, Cd = p.shape
    pc = np.maximum(np.concatenate([p, np.cumsum(p, axis=0) / np.arange(1, E + 1, dtype=np.float64)[:, None, None]]), 1e-256)
    pred = pc.argmax(axis=2)                                                     # [R, N]
    at_pred = np.take_along_axis(t["pkeys"], pred[:, None, :], axis=1)[:, 0, :]
    assert np.array_equal(at_pred, top["keys"])                                  # bit for bit
    assert (t["pkeys"] <= ONE).all() and (at_pred >= np.float32(1.0 / Cd).view(np.uint32) - 1).all()
    assert (t["count"].sum(-1) == t["valid"][:, None]).all() and (t["valid"] == N).all()
    assert np.array_equal(t["hits"].sum(-1), np.broadcast_to(np.bincount(y, minlength=Cd), (2 * E, Cd)))
    m = classwise_metrics(t)
    assert np.array_equal(m["class_count"], t["hits"].sum(-1))


def test_zeros_ones_and_the_flush():
    p, y, t = restated(CASES[4])                                                 # the first 75 images are one-hot on the label
    k = 75
    for n in range(0, k, 7):
        col = t["pkeys"][:, :, n]
        assert (col[:, y[n]] == ONE).all() and (np.delete(col, y[n], axis=1) == 0).all()
    c = int(y[0])
    line, other = t["pkeys"][0, c], t["pkeys"][0, (c + 1) % 100]
    zeros = int((other == 0).sum())
    assert zeros >= k - (y[:k] == (c + 1) % 100).sum() and t["count"][0, (c + 1) % 100, 0] >= zeros      # key 0 is counted, in bin 0
    filled = np.nonzero(t["count"][0, c])[0]
    assert t["count"][0, c, filled[-1]] >= (line == ONE).sum() >= 1 and filled[-1] == 14                  # 1.0f in the last bin
    # the flush: an explicit compare on the double at 2^-126
    tiny = np.array([[[1.0, 1e-40], [1.0, 2.0 ** -126], [1.0, 2.0 ** -126 * (1 - 2.0 ** -40)], [1.0, 0.0]]])
    f = classwise_numpy(tiny, np.zeros(4, dtype=np.int64), 2)
    assert f["pkeys"][0, 1].tolist() == [0, 0x00800000, 0, 0] and (f["pkeys"][0, 0] == ONE).all()
    assert f["count"][0, 1].tolist() == [4, 0] and f["conf_fix"][0, 1].tolist() == [0, 0] and f["valid"].tolist() == [4, 4]


def test_fixed_edges_with_a_threshold():
    p, y, full = restated(CASES[4])
    t = restated(CASES[4], binning="edges", edges=THRESHOLD_EDGES)[2]
    E, N, Cd = p.shape
    ed = np.asarray(THRESHOLD_EDGES, dtype=np.float32)
    assert t["edges"].shape == (2 * E, Cd, 6) and (t["edges"] == ed).all()
    conf = t["pkeys"].view(np.float32)
    assert np.array_equal(t["count"].sum(-1), (conf >= ed[0]).sum(-1)) and (t["count"].sum(-1) < N).any()   # pairs below edges[0]: in no bin
    assert np.array_equal(t["count"][..., 0], ((conf >= ed[0]) & (conf <= ed[1])).sum(-1))                   # bin 0 closed below
    assert np.array_equal(t["valid"], full["valid"]) and np.array_equal(t["pkeys"], full["pkeys"])
    for bad in ([0.0, 0.5, 0.4], [0.0, float("nan")], [0.5]):
        with pytest.raises(ValueError):
            classwise_numpy(p, y, binning="edges", edges=bad)
    with pytest.raises(ValueError):
        classwise_numpy(p, y, binning="edges")
    with pytest.raises(ValueError):
        classwise_numpy(p, y, binning="kde")


def test_non_finite_rows_and_bad_labels():
    p, y = make_case(3, 11, 10, 3, 9, 0)
    base = classwise_numpy(p, y)
    bad, yb = p.copy(), y.copy()
    bad[1, 2, 3] = np.nan
    bad[0, 4, :] = np.inf
    bad[2, 5, 0] = -np.inf
    yb[7], yb[8] = -1, 10
    dead = np.zeros((6, 11), dtype=bool)
    dead[[1, 4, 5], 2] = dead[[0, 3, 4, 5], 4] = dead[[2, 5], 5] = True         # a NaN in exit e: exit e and the ensembles e .. E - 1
    dead[:, 7] = dead[:, 8] = True
    for binning in ("width", "mass"):
        t = classwise_numpy(bad, yb, 15, binning)
        assert t["badlabel"] == 2 and t["nonfinite"] == (1 + 2) + (1 + 3) + (1 + 1)
        assert t["labels"].tolist() == [(-1 if n in (7, 8) else int(y[n])) for n in range(11)]
        assert (t["pkeys"].transpose(0, 2, 1)[dead] == INVALID).all()
        assert np.array_equal(t["pkeys"].transpose(0, 2, 1)[~dead], base["pkeys"].transpose(0, 2, 1)[~dead])
        assert np.array_equal(t["valid"], 11 - dead.sum(1))
        for name in ("edges", "count", "hits", "conf_fix", "valid"):
            assert np.isfinite(t[name]).all(), name
        assert (t["count"].sum(-1) == t["valid"][:, None]).all()
        want = np.stack([np.bincount(yb[~dead[r]], minlength=10) for r in range(6)])
        assert np.array_equal(t["hits"].sum(-1), want)
    # by mass the INVALID keys sort last, and an edge selected among them is 1.0: row 5 has 6 valid keys of 11, per = 11 // 4 = 2
    t = classwise_numpy(bad, yb, 4, "mass")
    srt = np.sort(t["pkeys"][5, 0])
    assert (srt[6:] == INVALID).all() and (srt[:6] != INVALID).all()
    assert t["edges"][5, 0].tolist() == [0.0, float(srt[2].view(np.float32)), float(srt[4].view(np.float32)), 1.0, 1.0]


def test_classwise_metrics_against_a_direct_computation():
    """The direct value from the float32 confidences in float64; 1e-10: the truncation is below 2^-40 = 9.1e-13 per pair — after the
    division by ``valid`` at most that per class —, and float64 rounding of fewer than 2^14 terms is below that."""
    for case in (CASES[4], CASES[1]):
        p, y, t = restated(case)
        m = classwise_metrics(t)
        E, N, Cd = p.shape
        conf = t["pkeys"].view(np.float32).astype(np.float64)
        ed = t["edges"].astype(np.float64)
        ece = np.zeros((2 * E, Cd))
        mce = np.zeros((2 * E, Cd))
        for r in range(2 * E):
            for c in range(Cd):
                hit = (y == c).astype(np.float64)
                for i in range(15):
                    sel = ((conf[r, c] >= ed[r, c, 0]) if i == 0 else (conf[r, c] > ed[r, c, i])) & (conf[r, c] <= ed[r, c, i + 1])
                    if sel.any():
                        acc, cf = hit[sel].mean(), conf[r, c][sel].mean()
                        ece[r, c] += abs(acc - cf) * sel.sum() / N
                        mce[r, c] = max(mce[r, c], abs(acc - cf))
        assert m["cw_ece_per_class"].shape == (2 * E, Cd) and m["cw_ece"].shape == (2 * E,)
        print(f"{case}: max |cw_ece_per_class - direct| = {np.abs(m['cw_ece_per_class'] - ece).max():.2e}")
        np.testing.assert_allclose(m["cw_ece_per_class"], ece, rtol=0, atol=1e-10)
        np.testing.assert_allclose(m["cw_ece"], ece.mean(1), rtol=0, atol=1e-10)
        np.testing.assert_allclose(m["cw_mce"], mce, rtol=0, atol=1e-10)
    empty = dict(t, valid=np.zeros_like(t["valid"]))
    assert np.isnan(classwise_metrics(empty)["cw_ece"]).all() and np.isnan(classwise_metrics(empty)["cw_ece_per_class"]).all()


def test_a_table_worked_by_hand():
    """Three images, two classes, one exit, two equal-width bins [0, 0.5], (0.5, 1]; labels 0, 1, 1:
        image   p           conf of class 0    conf of class 1
        0       0.75 0.25   0.75               0.25
        1       0.5  0.5    0.5                0.5
        2       0.0  1.0    0 (1e-256 / 1.0: flushed)   1.0
    class 0: bin 0 holds images 1, 2 (count 2, no label 0: hits 0, conf 0.5), bin 1 image 0 (count 1, hits 1, conf 0.75)
    class 1: bin 0 holds images 0, 1 (count 2, image 1 has label 1: hits 1, conf 0.75), bin 1 image 2 (count 1, hits 1, conf 1.0)
    classwise ECE: class 0 (|0 - 0.5| + |1 - 0.75|) / 3 = 1/4, class 1 (|1 - 0.75| + |1 - 1|) / 3 = 1/12, mean 1/6
    classwise MCE: class 0 max(|0/2 - 0.5/2|, |1 - 0.75|) = 1/4, class 1 max(|1/2 - 0.75/2|, 0) = 1/8"""
    p = np.array([[[0.75, 0.25], [0.5, 0.5], [0.0, 1.0]]])
    t = classwise_numpy(p, np.array([0, 1, 1]), 2)
    unit = 2 ** 40
    for r in (0, 1):                                                             # the exit, and the ensemble of it alone
        assert t["pkeys"][r].view(np.float32).tolist() == [[0.75, 0.5, 0.0], [0.25, 0.5, 1.0]]
        assert t["count"][r].tolist() == [[2, 1], [2, 1]] and t["hits"][r].tolist() == [[0, 1], [1, 1]]
        assert t["conf_fix"][r].tolist() == [[unit // 2, 3 * unit // 4], [3 * unit // 4, unit]]
    assert t["valid"].tolist() == [3, 3] and t["edges"][0, 1].tolist() == [0.0, 0.5, 1.0]
    m = classwise_metrics(t)
    np.testing.assert_allclose(m["cw_ece_per_class"], [[1 / 4, 1 / 12]] * 2, rtol=1e-15)
    np.testing.assert_allclose(m["cw_ece"], [1 / 6] * 2, rtol=1e-15)
    assert m["cw_mce"].tolist() == [[0.25, 0.125]] * 2 and m["class_count"].tolist() == [[1, 2]] * 2
    assert FIX == float(unit)
