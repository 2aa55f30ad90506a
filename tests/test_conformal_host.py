"""Conformal prediction sets without a GPU: the ctypes bindings, the restatement ``conformal_numpy`` against a plain reference written here
(a stable descending argsort of the keys, ties by class index, and a cumulative sum of Python-exact integers) — every output, exact
equality —, and the invariant that the sets of the calibration records under their own quantile cover at least k labels."""
import math

import numpy as np
import pytest

from bayesnn_fpga_amd import _lib
from bayesnn_fpga_amd.train.conformal import conformal_metrics, conformal_numpy
from bayesnn_fpga_amd.train.reliability import classwise_numpy

INVALID, MAX_KEY = 0xFFFFFFFF, 0xFFFFFFFE
# (method, k_reg, lam): the last one saturates the key at C = 128
METHODS = [("lac", 0, 0.0), ("aps", 0, 0.0), ("raps", 1, 0.01), ("raps", 5, 1.0)]
COVERAGE = (0.5, 0.9, 0.999)                 # at N <= 200 the last level has k > n: the quantile that admits every class
SHAPES = [(C_, E, N) for C_ in (1, 10, 65, 128) for E in (1, 3) for N in (1, 64, 65, 200)]
IDS = dict(ids=lambda s: "C{}E{}N{}".format(*s))
OUTPUTS = ("score_keys", "qhat", "n_valid", "set_size", "members", "valid", "covered", "size_sum", "size_hist", "cov_hist", "class_n", "class_cov")
_seen = {}


def make_inputs(C_, E, N):
    """(mean float64 [E, N, C], labels int64 [N], classwise_numpy of them): eight eighths thrown at the classes — equal keys inside an image
    —, image 0 exactly uniform, half the labels at exit 0's arg-max; from three images on a NaN in exit 0 of image 1 and the label C at 2."""
    if (C_, E, N) not in _seen:
        rng = np.random.default_rng(1000 * C_ + 10 * N + E)
        p = rng.multinomial(8, np.full(C_, 1.0 / C_), size=(E, N)) / 8.0
        p[:, 0] = 1.0 / C_
        y = np.where(rng.random(N) < 0.5, p[0].argmax(1), rng.integers(0, C_, N))
        if N > 2:
            p[0, 1, 0], y[2] = np.nan, C_
        _seen[C_, E, N] = (p, y, classwise_numpy(p, y))
    return _seen[C_, E, N]


def reference(pkeys, labels, method, k_reg, lam, coverage, qhat=None):
    """The three calls, plainly: per row a stable argsort of the negated keys, a cumulative sum in that order, the sorted label scores"""
    R, Cd, N = pkeys.shape
    L, lam_fix = len(coverage), int(lam * 2 ** 30)
    ok = (pkeys != INVALID).all(1) & (labels >= 0) & (labels < Cd)                           # [R, N]
    u = (np.where(pkeys == INVALID, 0, pkeys).astype(np.uint32).view(np.float32).astype(np.float64) * 2.0 ** 30).astype(np.uint64)
    order = np.argsort(-pkeys.astype(np.int64), axis=1, kind="stable")                       # descending key, ties by class index
    cum = np.cumsum(np.take_along_axis(u, order, 1), axis=1, dtype=np.uint64)
    if method == "raps":
        cum = cum + np.uint64(lam_fix) * np.maximum(np.arange(Cd) + 1 - k_reg, 0).astype(np.uint64)[None, :, None]
    score = np.empty_like(cum)
    np.put_along_axis(score, order, cum, 1)
    if method == "lac":
        score = np.uint64(2 ** 30) - u
    keys = np.where(ok[:, None, :], np.minimum(score, np.uint64(MAX_KEY)), INVALID).astype(np.uint32)
    out = dict(score_keys=np.where(ok, keys[:, np.clip(labels, 0, Cd - 1), np.arange(N)], INVALID).astype(np.uint32),
               n_valid=ok.sum(1), valid=ok.sum(1), qhat=np.full((R, L), MAX_KEY, dtype=np.uint32), k=np.zeros((R, L), dtype=np.int64),
               set_size=np.full((R, L, N), 255, dtype=np.uint8), members=np.zeros((R, L, (Cd + 31) // 32, N), dtype=np.uint32),
               class_n=np.zeros((R, Cd), dtype=np.int64), **{k: np.zeros((R, L), dtype=np.int64) for k in ("covered", "size_sum")},
               **{k: np.zeros((R, L, Cd + 1), dtype=np.int64) for k in ("size_hist", "cov_hist")}, class_cov=np.zeros((R, L, Cd), dtype=np.int64))
    for r in range(R):
        line, n = sorted(out["score_keys"][r][ok[r]].tolist()), int(ok[r].sum())
        for l, q in enumerate(coverage):
            out["k"][r, l] = k = math.ceil((n + 1) * q)
            if 0 < k <= n:
                out["qhat"][r, l] = line[k - 1]
    for r, l, n in np.ndindex(R, L, N):
        if ok[r, n]:
            inside = keys[r, :, n] <= (out["qhat"] if qhat is None else qhat)[r, l]
            size, hit, c = int(inside.sum()), bool(inside[labels[n]]), int(labels[n])
            out["members"][r, l, :, n] = np.packbits(np.pad(inside, (0, -Cd % 32)), bitorder="little").view(np.uint32)
            out["set_size"][r, l, n] = size
            out["size_hist"][r, l, size] += 1
            out["size_sum"][r, l] += size
            out["class_n"][r, c] += l == 0
            for name, at in (("covered", (r, l)), ("cov_hist", (r, l, size)), ("class_cov", (r, l, c))):
                out[name][at] += hit
    return out


def expected(shape, method):
    """(pkeys uint32 [R, C, N], label records, the reference's outputs): computed once per (shape, method)"""
    if (shape, method) not in _seen:
        t = make_inputs(*shape)[2]
        _seen[shape, method] = (t["pkeys"], t["labels"], reference(t["pkeys"], t["labels"], *method, COVERAGE))
    return _seen[shape, method]


def test_lib_declares_the_entry_points_and_the_abi_version_stays():
    for name in ("bmi_conformal_scores", "bmi_conformal_quantile", "bmi_conformal_sets"):
        assert name in _lib.EXPORTS and hasattr(_lib.lib(), name)
    assert _lib.ABI_VERSION == 600 and _lib.lib().bmi_version() == 600


@pytest.mark.parametrize("method", METHODS, ids=lambda m: "{}-{}-{}".format(*m))
@pytest.mark.parametrize("shape", SHAPES, **IDS)
def test_numpy_restatement_equals_the_plain_reference(shape, method):
    pkeys, labels, want = expected(shape, method)
    got = conformal_numpy(pkeys, labels, *method, COVERAGE)
    for name in OUTPUTS + ("k",):
        assert got[name].shape == want[name].shape and np.array_equal(got[name], want[name]), name
    if shape == (128, 3, 200) and method == ("raps", 5, 1.0):
        assert (got["class_keys"] == MAX_KEY).any()                                          # the key saturates
    if shape[2] > 2:
        assert (got["score_keys"][:, 2] == INVALID).all() and got["score_keys"][0, 1] == INVALID and (got["set_size"][:, :, 2] == 255).all()
    assert (got["qhat"][:, 2] == MAX_KEY).all() and (got["k"][:, 2] > got["n_valid"]).all()   # 0.999: too few images for the level
    assert (got["set_size"][:, 2][got["set_size"][:, 2] != 255] == shape[0]).all()           # ... so every class is in every set


@pytest.mark.parametrize("method", METHODS, ids=lambda m: "{}-{}-{}".format(*m))
def test_the_calibration_records_are_covered_k_times_under_their_own_quantile(method):
    """Exact, not statistical: at least k labels have a score key at or below the order statistic of rank k - 1"""
    for shape in ((10, 3, 200), (128, 1, 65)):
        got = conformal_numpy(*expected(shape, method)[:2], *method, COVERAGE)
        reached = got["k"] <= got["n_valid"][:, None]
        assert reached[:, :2].all() and (got["covered"] >= got["k"])[reached].all()
        m = conformal_metrics(got)
        assert np.array_equal(m["coverage"], got["covered"] / got["valid"][:, None].astype(np.float64)) and (m["coverage"][:, 2] == 1.0).all()
        assert (m["worst_size_coverage"] <= m["coverage"]).all() and (m["worst_class_coverage"] <= m["coverage"]).all()
        assert np.array_equal(m["mean_size"], got["size_sum"] / got["valid"][:, None].astype(np.float64))
