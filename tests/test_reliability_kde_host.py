"""The KDE-ECE without a GPU: the float64 restatement ``reliability_kde_numpy`` of bmi_reliability_kde's contract against the host estimators
``train.metrics.ece_kde_binary`` (exact densities within 1e-7, the FFT approximation within 1e-6 on the 2^14-point grid), every path of the
contract asserted from the restatement's intermediate arrays, the degenerate rows, the bindings and the C ABI's host-side validation (no
call reaches a kernel)."""
import ctypes as C

import numpy as np
import pytest

from bayesnn_fpga_amd import _lib
from bayesnn_fpga_amd.train.metrics import ece_kde_binary
from bayesnn_fpga_amd.train.reliability import kde_bw_scale, reliability_kde_numpy, reliability_numpy

# (N, C, G, sharpness, seed, lift): softmax of normal logits times the sharpness, the label's logit raised by lift * sharpness
CASES = [(300, 10, 1024, 2.0, 0, 1.2), (300, 3, 1024, 1.5, 1, 1.2), (1000, 100, 2 ** 14, 3.0, 2, 2.5), (1000, 10, 2 ** 14, 2.0, 3, 1.2),
         (3000, 10, 2 ** 14, 2.5, 4, 1.2)]
DIRECT_BOUND, FFT_BOUND = 1e-7, 1e-6
IDS = dict(ids=lambda c: "N{}C{}G{}".format(*c[:3]))
OUTPUTS = ("ece_kde", "bw", "sd", "n_data", "n_hit", "degenerate", "density")


def make_probs(N, C_, sharp, seed, lift=1.2):
    """-> (p float64 [N, C], labels int64 [N]): accuracy between 0.25 and 0.75 (asserted by the tests that rely on it)"""
    rng = np.random.default_rng(seed)
    l = rng.standard_normal((N, C_)) * sharp
    y = rng.integers(0, C_, N)
    l[np.arange(N), y] += lift * sharp
    ex = np.exp(l - l.max(-1, keepdims=True))
    return ex / ex.sum(-1, keepdims=True), y


def onehot(y, C_):
    o = np.zeros((len(y), C_))
    o[np.arange(len(y)), y] = 1
    return o


def records_of(p, y):
    """The keys and hit bits of ONE row (exit 0) as bmi_reliability_record forms them"""
    t = reliability_numpy(np.asarray(p, dtype=np.float64)[None], y)
    return t["keys"][:1], t["hit"][:1]


def records_from(conf, hit):
    """Records of one row from float32 confidences (0: no datum) and hit bits"""
    return np.asarray(conf, dtype=np.float32).view(np.uint32)[None].copy(), np.asarray(hit, dtype=np.uint8)[None].copy()


def probs_with_conf(conf, hit):
    """Four-class probabilities whose top-label confidence is ``conf`` (float32 values above 0.25, on class 0) -> (p float64 [N, 4], labels)"""
    c = np.asarray(conf, dtype=np.float32).astype(np.float64)
    return np.stack([c] + [(1.0 - c) / 3.0] * 3, axis=1), np.where(np.asarray(hit, dtype=bool), 0, 1)


_seen = {}


def restated(case):
    """(p, labels, keys, hit, reliability_kde_numpy of them): computed once per case"""
    if case not in _seen:
        N, C_, G, sharp, seed, lift = case
        p, y = make_probs(N, C_, sharp, seed, lift)
        keys, hit = records_of(p, y)
        _seen[case] = (p, y, keys, hit, reliability_kde_numpy(keys, hit, N, G))
    return _seen[case]


@pytest.mark.parametrize("case", CASES, **IDS)
def test_restatement_against_the_host_estimators(case):
    N, C_, G = case[:3]
    p, y, keys, hit, t = restated(case)
    acc = hit[0].mean()
    assert 0.25 <= acc <= 0.75 and t["degenerate"][0] == 0 and t["n_data"][0] == N and t["n_hit"][0] == hit[0].sum()
    assert t["bw"][0] == t["sd"][0] * kde_bw_scale(N) and t["h"][0] == 3.0 * t["bw"][0] and t["density"].shape == (1, 2, G)
    direct = ece_kde_binary(p, onehot(y, C_), grid_points=G, method="direct")
    print(f"{case}: ece_kde = {t['ece_kde'][0]:.9f}, |restatement - direct| = {abs(t['ece_kde'][0] - direct):.2e}")
    assert abs(t["ece_kde"][0] - direct) <= DIRECT_BOUND
    if G == 2 ** 14:                                         # (at G = 1024 the binning error is the FFT method's own)
        fft = ece_kde_binary(p, onehot(y, C_), grid_points=G, method="fft")
        print(f"{case}: |restatement - fft| = {abs(t['ece_kde'][0] - fft):.2e}")
        assert abs(t["ece_kde"][0] - fft) <= FFT_BOUND
    # the densities are the reference's: each integrates to about 1 over (0, 1), and the grid is numpy's linspace
    assert np.array_equal(t["x"][:-1], np.linspace(-0.6, 1.6, G)[:-1]) and not 0.0 < t["x"][-1] < 1.0
    assert abs(t["b"][0] - 1.0) < 0.02


def test_order_two():
    N, C_, G = CASES[0][:3]
    p, y, keys, hit, one = restated(CASES[0])
    two = reliability_kde_numpy(keys, hit, N, G, order=2)
    direct = ece_kde_binary(p, onehot(y, C_), order=2, grid_points=G, method="direct")
    print(f"order 2: |restatement - direct| = {abs(two['ece_kde'][0] - direct):.2e}")
    assert abs(two["ece_kde"][0] - direct) <= DIRECT_BOUND
    assert np.array_equal(two["density"], one["density"]) and two["ece_kde"][0] < one["ece_kde"][0]
    s = two["is_set"][0]
    gap1, gap2 = one["integrand"][0][s] / one["density"][0, 1][s], two["integrand"][0][s] / two["density"][0, 1][s]
    np.testing.assert_allclose(gap2, gap1 * gap1, rtol=1e-12, atol=1e-300)


def test_tied_two_class_probabilities_mirror_upwards():
    """C = 2 with tied probabilities: the confidence is exactly 0.5, whose mirror is 2 - d = 1.5, not -0.5"""
    p, y = make_probs(200, 2, 1.0, 5, lift=0.3)
    p[:40] = 0.5
    keys, hit = records_of(p, y)
    t = reliability_kde_numpy(keys, hit, 200, 1024)
    conf = keys[0].view(np.float32)
    assert (conf[:40] == 0.5).all() and t["mirror_high"][0, :40].all() and t["mirror_high"][0].all()       # C = 2: every confidence >= 0.5
    assert hit[0, :40].tolist() == (y[:40] == 0).astype(int).tolist()                                     # the tie goes to class 0
    direct = ece_kde_binary(p, onehot(y, 2), grid_points=1024, method="direct")
    print(f"tied C = 2: |restatement - direct| = {abs(t['ece_kde'][0] - direct):.2e}")
    assert t["degenerate"][0] == 0 and abs(t["ece_kde"][0] - direct) <= DIRECT_BOUND
    # a mirror at -0.5 would put mass left of 0.5 - h; there is none
    x, h = t["x"], t["h"][0]
    assert h < 0.25 and (t["sums"][0, 1][x < conf.min() - h] == 0).all() and t["sums"][0, 1][np.abs(x - 1.5) < h / 2].min() > 0


def test_saturated_images_and_both_mirrors():
    """Confidence exactly 1.0 (mirror 1.0: the centre counts twice) and confidences below 0.5 (mirror -d)"""
    p, y = make_probs(300, 10, 1.0, 6, lift=1.5)
    p[:30] = 0.0
    p[np.arange(30), y[:30]] = 1.0
    keys, hit = records_of(p, y)
    t = reliability_kde_numpy(keys, hit, 300, 1024)
    conf = keys[0].view(np.float32)
    assert (conf[:30] == 1.0).all() and hit[0, :30].all() and (conf < 0.5).any() and not t["mirror_high"][0][conf < 0.5].any()
    direct = ece_kde_binary(p, onehot(y, 10), grid_points=1024, method="direct")
    print(f"saturated: |restatement - direct| = {abs(t['ece_kde'][0] - direct):.2e}")
    assert abs(t["ece_kde"][0] - direct) <= DIRECT_BOUND
    assert np.isfinite(t["density"]).all() and t["density"][0, 0][t["x"] < 1.0].max() > 0


def two_clusters(N=2000, seed=7):
    """Confidences near 0.35 (one in ten right) and near 0.95 (nine in ten right), float32, with hit bits: few of the hits are low, so the
    bandwidth stays narrow — h is about 0.09 — and no kernel reaches the grid points between 0.5 and 0.8"""
    rng = np.random.default_rng(seed)
    low = rng.random(N) < 0.4
    conf = np.where(low, 0.35 + 0.01 * rng.standard_normal(N), 0.95 + 0.01 * rng.standard_normal(N)).astype(np.float32)
    hit = np.where(low, rng.random(N) < 0.1, rng.random(N) < 0.9)
    return conf, hit


def test_carry_forward_across_an_interior_gap():
    conf, hit = two_clusters()
    keys, hb = records_from(conf, hit)
    t = reliability_kde_numpy(keys, hb, len(conf), 2048)
    x, s, I = t["x"], t["is_set"][0], t["integrand"][0]
    assert t["h"][0] < 0.1 and t["degenerate"][0] == 0
    gap = (x > 0.5) & (x < 0.8)
    assert not s[gap].any() and (I[gap] > 0).all()                               # carried, and not zero
    first = np.nonzero(gap)[0][0]
    src = np.nonzero(s[:first])[0][-1]
    assert (I[gap] == I[src]).all() and 0.35 < x[src] < 0.5
    assert s[(x > 0.34) & (x < 0.36)].all() and s[(x > 0.94) & (x < 0.96)].all()
    # the loop of ece_kde_binary on the same densities gives the same value (its confidences are these float32 ones here)
    p, y = probs_with_conf(conf, hit)
    direct = ece_kde_binary(p, onehot(y, 4), grid_points=2048, method="direct")
    print(f"two clusters: |restatement - direct| = {abs(t['ece_kde'][0] - direct):.2e}")
    assert abs(t["ece_kde"][0] - direct) <= DIRECT_BOUND


DEGENERATE = {
    "no hit": ([0.3, 0.6, 0.9, 0.7], [0, 0, 0, 0]),
    "one hit": ([0.3, 0.6, 0.9, 0.7], [0, 1, 0, 0]),
    "equal hit confidences": ([0.3, 0.75, 0.75, 0.75, 0.4], [0, 1, 1, 1, 0]),
    "all records invalid": ([0.0, 0.0, 0.0], [0, 0, 0]),
}


@pytest.mark.parametrize("kind", DEGENERATE)
def test_degenerate_rows(kind):
    conf, hit = DEGENERATE[kind]
    keys, hb = records_from(conf, hit)
    t = reliability_kde_numpy(keys, hb, len(conf), 1024)
    assert t["degenerate"][0] == 1 and t["ece_kde"][0] == 0.0 and t["sd"][0] == 0.0 and t["bw"][0] == 1e-16 * kde_bw_scale(len(conf))
    assert t["n_data"][0] == np.count_nonzero(conf) and t["n_hit"][0] == sum(hit)
    assert all(np.isfinite(t[k]).all() for k in OUTPUTS) and (t["density"] == 0).all()
    if kind != "all records invalid":                        # the host estimator's answer there is NaN
        p, y = probs_with_conf(conf, hit)
        with np.errstate(invalid="ignore", divide="ignore"):
            assert np.isnan(ece_kde_binary(p, onehot(y, 4), grid_points=1024, method="direct"))


def test_records_with_key_zero_are_ignored():
    N, C_, G = CASES[0][:3]
    _, _, keys, hit, t = restated(CASES[0])
    k2 = np.zeros((1, N + 50), dtype=np.uint32)
    h2 = np.ones((1, N + 50), dtype=np.uint8)                # a hit bit beside a zero key counts for nothing
    at = np.sort(np.random.default_rng(0).choice(N + 50, N, replace=False))
    k2[0, at], h2[0, at] = keys[0], hit[0]
    t2 = reliability_kde_numpy(k2, h2, N + 50, G, bw_scale=kde_bw_scale(N))
    for k in OUTPUTS:
        assert np.array_equal(t2[k], t[k]), k
    # columns beyond n are not read
    t3 = reliability_kde_numpy(np.concatenate([keys, keys[:, :7]], axis=1), np.concatenate([hit, 1 - hit[:, :7]], axis=1), N, G)
    assert all(np.array_equal(t3[k], t[k]) for k in OUTPUTS)
    for bad in (dict(grid_points=15), dict(grid_points=65537), dict(order=3), dict(bw_scale=0.0), dict(bw_scale=float("inf"))):
        with pytest.raises(ValueError):
            reliability_kde_numpy(keys, hit, N, **{"grid_points": G, **bad})


def test_lib_declares_the_entry_point_and_the_abi_version_stays():
    assert "bmi_reliability_kde" in _lib.EXPORTS and hasattr(_lib.lib(), "bmi_reliability_kde")
    assert _lib.ABI_VERSION == 600 and _lib.lib().bmi_version() == 600
    assert (_lib.KDE_MIN_GRID, _lib.KDE_MAX_GRID) == (16, 65536)


def test_c_abi_validation():
    """Null pointers, counts below 1, N beyond the capacity, the grid's range, the order, bw_scale and the shape limits: decided on the
    host, before any launch (the device pointers are never dereferenced)."""
    lib, fake = _lib.lib(), C.c_void_p(4096)
    INVALID, UNSUPPORTED = -22, -95
    ok = [fake, fake, 8, 1000, 1003, 1024, 1, 0.2] + [fake] * 7 + [None]
    for i in (0, 1, 8, 9, 10, 11, 12, 13, 14):
        args = list(ok)
        args[i] = None
        assert lib.bmi_reliability_kde(*args) == INVALID, i
    for i, values in ((2, (0, -1)), (3, (0, -1, 1004)), (5, (15, 0, -1, 65537)), (6, (0, 3, -1)),
                      (7, (0.0, -0.2, float("nan"), float("inf"), -float("inf")))):
        for v in values:
            args = list(ok)
            args[i] = v
            assert lib.bmi_reliability_kde(*args) == INVALID, (i, v)
    for i, v in ((2, 65), (7, 2.0 ** -101), (7, 2.0 ** 101)):
        args = list(ok)
        args[i] = v
        assert lib.bmi_reliability_kde(*args) == UNSUPPORTED, (i, v)
    args = list(ok)
    args[3], args[4] = 1 << 22, 1 << 22
    assert lib.bmi_reliability_kde(*args) == UNSUPPORTED
