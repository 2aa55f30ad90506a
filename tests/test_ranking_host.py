"""Rank quality without a GPU: the restatements ``score_keys_numpy`` / ``rank_quality_numpy`` of csrc/ranking.hip's contract against a
brute-force double loop over the pairs (exact integers) and scikit-learn's AUROC, the key encoding, ties, invalid and spare columns, the
degenerate rows, the curve read-outs, the bindings and the C ABI's host-side validation (no call reaches a kernel)."""
import ctypes as C

import numpy as np
import pytest

from bayesnn_fpga_amd import _lib
from bayesnn_fpga_amd.train.ranking import (INVALID, MAX_KEY, rank_metrics, rank_quality_numpy, risk_at_coverage, score_keys_numpy,
                                            threshold_at_coverage)

OUTPUTS = ("rank", "sorted_keys", "curve", "counts", "aurc_sum")
SIZES = (2, 65, 257, 4097, 5000)
AUROC_BOUND = 1e-12           # both sides are float64 sums of at most a few thousand terms


def make_scores(N, seed, ties):
    """-> (score float64 [N], positive uint8 [N]): the positives score higher on average; ``ties``: twelve score levels"""
    rng = np.random.default_rng(seed)
    pos = (rng.random(N) < 0.3).astype(np.uint8)
    if N >= 2:
        pos[0], pos[1] = 0, 1
    s = rng.random(N) + 0.4 * pos
    return (np.floor(s * 8) / 8 if ties else s), pos


def brute(u, pos):
    """The contract by a double loop over the pairs of ONE row -> (rank, curve by position, U2)"""
    n = len(u)
    valid = [v != INVALID for v in u]
    rank = np.full(n, -1, dtype=np.int64)
    curve = {}
    u2 = 0
    for i in range(n):
        if not valid[i]:
            continue
        less = eq_before = less_pos = eq_pos_before = 0
        for j in range(n):
            if not valid[j]:
                continue
            if u[j] < u[i]:
                less += 1
                less_pos += int(pos[j])
                u2 += 2 * int(pos[i] and not pos[j])
            elif u[j] == u[i]:
                u2 += int(pos[i] and not pos[j])
                if j < i:
                    eq_before += 1
                    eq_pos_before += int(pos[j])
        rank[i] = less + eq_before
        curve[rank[i]] = less_pos + eq_pos_before + int(pos[i])
    return rank, curve, u2


@pytest.mark.parametrize("ties", (False, True), ids=("distinct", "ties"))
@pytest.mark.parametrize("N", (1, 2, 65, 257))
def test_restatement_against_the_double_loop(N, ties):
    s, pos = make_scores(N, N, ties)
    s[N // 3::17] = np.nan                                   # a few invalid images
    u, bad = score_keys_numpy(s[None], 1)
    t = rank_quality_numpy(u, pos[None], N)
    rank, curve, u2 = brute(u[0].tolist(), pos.tolist())
    m = int((u[0] != INVALID).sum())
    assert bad == N - m and t["counts"][0].tolist() == [m, int(pos[u[0] != INVALID].sum()), u2]
    assert t["rank"][0].tolist() == rank.tolist() and sorted(rank[rank >= 0].tolist()) == list(range(m))
    assert t["curve"][0, :m].tolist() == [curve[k] for k in range(m)] and (t["curve"][0, m:] == t["counts"][0, 1]).all()
    order = np.argsort(np.where(u[0] == INVALID, 2 ** 40, u[0].astype(np.int64)), kind="stable")[:m]
    assert t["sorted_keys"][0, :m].tolist() == u[0][order].tolist() and (t["sorted_keys"][0, m:] == INVALID).all()
    want = 0.0
    for k in range(m):
        want = want + float(curve[k]) / float(k + 1)
    assert t["aurc_sum"][0] == want


@pytest.mark.parametrize("ties", (False, True), ids=("distinct", "ties"))
@pytest.mark.parametrize("N", SIZES)
def test_auroc_against_scikit_learn(N, ties):
    metrics = pytest.importorskip("sklearn.metrics")
    s, pos = make_scores(N, 100 + N, ties)
    s = s.astype(np.float32).astype(np.float64)              # (the keys hold the float32 score: both sides rank the same numbers)
    u, bad = score_keys_numpy(s[None], 1)
    m = rank_metrics(rank_quality_numpy(u, pos[None], N))
    ref = metrics.roc_auc_score(pos, s)
    print(f"N = {N}, ties = {ties}: auroc = {m['auroc'][0]:.12f}, |ours - sklearn| = {abs(m['auroc'][0] - ref):.2e}")
    assert bad == 0 and abs(m["auroc"][0] - ref) <= AUROC_BOUND
    # a confidence ranks the other way round: 1 - score flags the same images under direction -1
    v, _ = score_keys_numpy(1.5 - s[None], -1)
    assert abs(rank_metrics(rank_quality_numpy(v, pos[None], N))["auroc"][0] - metrics.roc_auc_score(pos, -(1.5 - s))) <= AUROC_BOUND


def test_key_encoding():
    vals = np.array([0.0, 1e-45, 1e-38, 1e-3, 0.5, 1.0, 1.0 + 2.0 ** -23, 2.5, 3.0e38, 3.4028234663852886e38])     # ascending float32 values
    up, bad_up = score_keys_numpy(vals[None], 1)
    down, bad_down = score_keys_numpy(vals[None], -1)
    assert bad_up == bad_down == 0
    assert (np.diff(up[0].astype(np.int64)) > 0).all() and (np.diff(down[0].astype(np.int64)) < 0).all()
    assert up[0, 0] == 0 and up[0, -1] == MAX_KEY and down[0, 0] == MAX_KEY and down[0, -1] == 0
    assert np.array_equal(up[0].view(np.float32), vals.astype(np.float32)) and ((up + down) == MAX_KEY).all()
    zero, bad = score_keys_numpy(np.array([[-0.0, 0.0, -1e-60]]), 1)            # -1e-60 rounds to -0.0 in float32
    assert bad == 0 and zero[0].tolist() == [0, 0, 0]
    zero, bad = score_keys_numpy(np.array([[-0.0, 0.0]]), -1)
    assert bad == 0 and zero[0].tolist() == [MAX_KEY, MAX_KEY]
    for direction in (1, -1):
        k, bad = score_keys_numpy(np.array([[np.nan, np.inf, -np.inf, -1e-3, 1e39, 0.25]]), direction)    # 1e39 overflows float32
        assert bad == 5 and (k[0, :5] == INVALID).all() and k[0, 5] != INVALID
    # valid_keys == 0 silences an image, whatever its score, and is not counted
    k, bad = score_keys_numpy(np.array([[0.1, np.nan, 0.3, np.nan]]), 1, np.array([[7, 0, 0, 9]], dtype=np.uint32))
    assert bad == 1 and k[0].tolist() == [int(np.float32(0.1).view(np.uint32)), INVALID, INVALID, INVALID]
    for bad_direction in (0, 2, -2):
        with pytest.raises(ValueError):
            score_keys_numpy(vals[None], bad_direction)


def test_ties_are_broken_by_index():
    N = 37
    pos = (np.arange(N) % 3 == 0).astype(np.uint8)
    t = rank_quality_numpy(np.full((1, N), 12345, dtype=np.uint32), pos[None], N)
    assert t["rank"][0].tolist() == list(range(N)) and t["curve"][0].tolist() == np.cumsum(pos).tolist()
    n_pos = int(pos.sum())
    assert t["counts"][0].tolist() == [N, n_pos, n_pos * (N - n_pos)] and rank_metrics(t)["auroc"][0] == 0.5
    # two levels, interleaved: each level's images keep their order
    u = np.where(np.arange(N) % 2 == 0, 9, 5).astype(np.uint32)
    t = rank_quality_numpy(u[None], pos[None], N)
    assert t["rank"][0].tolist() == np.argsort(np.argsort(u, kind="stable"), kind="stable").tolist()


def test_invalid_and_spare_columns_are_ignored():
    N = 300
    s, pos = make_scores(N, 7, True)
    u, _ = score_keys_numpy(s[None], 1)
    t = rank_quality_numpy(u, pos[None], N)
    wide = np.full((1, N + 40), INVALID, dtype=np.uint32)
    wpos = np.ones((1, N + 40), dtype=np.uint8)              # a positive bit beside an invalid key counts for nothing
    at = np.sort(np.random.default_rng(0).choice(N + 40, N, replace=False))
    wide[0, at], wpos[0, at] = u[0], pos
    w = rank_quality_numpy(wide, wpos, N + 40)
    assert np.array_equal(w["counts"], t["counts"]) and w["aurc_sum"][0] == t["aurc_sum"][0]
    assert np.array_equal(w["rank"][0, at], t["rank"][0]) and (np.delete(w["rank"][0], at) == -1).all()
    assert np.array_equal(w["sorted_keys"][0, :N], t["sorted_keys"][0]) and (w["sorted_keys"][0, N:] == INVALID).all()
    assert np.array_equal(w["curve"][0, :N], t["curve"][0]) and (w["curve"][0, N:] == t["counts"][0, 1]).all()
    # columns beyond n are not read
    more = rank_quality_numpy(np.concatenate([u, u[:, :9]], axis=1), np.concatenate([pos[None], 1 - pos[None, :9]], axis=1), N)
    assert all(np.array_equal(more[k], t[k]) for k in OUTPUTS)
    for bad in (0, N + 1):
        with pytest.raises(ValueError):
            rank_quality_numpy(u, pos[None], bad)


def test_degenerate_rows():
    """No positive, no negative, no valid image: NaN in the metrics, finite numbers in the device-contract outputs"""
    N = 9
    u = np.arange(N, dtype=np.uint32)[None].repeat(3, axis=0)
    u[2] = INVALID
    pos = np.stack([np.zeros(N), np.ones(N), np.ones(N)]).astype(np.uint8)
    t = rank_quality_numpy(u, pos, N)
    assert t["counts"].tolist() == [[N, 0, 0], [N, N, 0], [0, 0, 0]]
    assert t["aurc_sum"].tolist() == [0.0, float(N), 0.0] and all(np.isfinite(t[k]).all() for k in ("aurc_sum", "counts", "curve"))
    assert (t["rank"][2] == -1).all() and (t["sorted_keys"][2] == INVALID).all() and (t["curve"][2] == 0).all()
    m = rank_metrics(t)
    assert np.isnan(m["auroc"]).all() and np.isnan(m["aurc"][2]) and np.isnan(m["eaurc"][2])
    assert m["aurc"][:2].tolist() == [0.0, 1.0] and m["eaurc"][:2].tolist() == [0.0, 0.0]
    assert np.isnan(risk_at_coverage(t, 0.5)[2]) and np.isnan(threshold_at_coverage(t, 0.5, 1)[2])
    assert risk_at_coverage(t, 0.5)[:2].tolist() == [0.0, 1.0]


@pytest.mark.parametrize("N,n_pos", ((10, 3), (257, 100), (1000, 1)))
def test_a_perfect_ranking_has_no_excess(N, n_pos):
    pos = np.zeros(N, dtype=np.uint8)
    pos[N - n_pos:] = 1
    perm = np.random.default_rng(N).permutation(N)
    u = np.empty(N, dtype=np.uint32)
    u[perm] = np.arange(N) * 3                               # image perm[k] is ranked k; the positives hold the highest keys
    p = np.empty(N, dtype=np.uint8)
    p[perm] = pos
    m = rank_metrics(rank_quality_numpy(u[None], p[None], N))
    assert m["auroc"][0] == 1.0 and m["eaurc"][0] == 0.0 and m["aurc"][0] > 0.0
    worst = rank_metrics(rank_quality_numpy((MAX_KEY - u)[None], p[None], N))
    assert worst["auroc"][0] == 0.0 and worst["eaurc"][0] > 0.0


def test_risk_and_threshold_at_coverage():
    N = 40
    s, pos = make_scores(N, 3, False)
    for direction, score in ((1, s), (-1, 2.0 - s)):
        u, _ = score_keys_numpy(score[None], direction)
        t = rank_quality_numpy(u, pos[None], N)
        order = np.argsort(s, kind="stable")
        f32 = score.astype(np.float32)
        for c, k in ((1.0 / N, 1), (0.5, N // 2), (1.0, N), (0.0, 1), (0.51, 21), (7.0, N)):
            assert risk_at_coverage(t, c)[0] == float(pos[order[:k]].sum()) / float(k), (direction, c)
            th = threshold_at_coverage(t, c, direction)
            assert th.dtype == np.float32 and th[0] == f32[order[k - 1]], (direction, c)
            kept = f32 <= th[0] if direction > 0 else f32 >= th[0]
            assert kept.sum() == k
    with pytest.raises(ValueError):
        threshold_at_coverage(t, 0.5, 0)


def test_lib_declares_the_entry_points_and_the_abi_version_stays():
    for name in ("bmi_score_record", "bmi_rank_quality", "bmi_rank_scratch_bytes"):
        assert name in _lib.EXPORTS and hasattr(_lib.lib(), name)
    assert _lib.ABI_VERSION == 600 and _lib.lib().bmi_version() == 600
    assert _lib.RANK_TILE_I >= 64 and _lib.RANK_TILE_J % _lib.RANK_TILE_I == 0
    assert (_lib.RANK_MAX_IMAGES, _lib.RANK_MAX_ROWS, _lib.RANK_INVALID, _lib.RANK_MAX_KEY) == (2 ** 17, 1024, INVALID, MAX_KEY)
    sb = _lib.lib().bmi_rank_scratch_bytes
    tiles = lambda n: -(-n // _lib.RANK_TILE_I)
    assert sb(8, 10000) == 8 * tiles(10000) * 24 and sb(1, 1) == 24 and sb(1024, 2 ** 17) == 1024 * tiles(2 ** 17) * 24
    assert sb(0, 5) == sb(5, 0) == sb(1025, 5) == sb(1, 2 ** 17 + 1) == sb(-1, -1) == 0


def test_c_abi_validation():
    """Null pointers, counts below 1, the offset and the capacity, the direction, the limits and the scratch size: decided on the host,
    before any launch (the device pointers are never dereferenced)."""
    lib, fake = _lib.lib(), C.c_void_p(4096)
    INVALID_, UNSUPPORTED, NOMEM = -22, -95, -12
    # bmi_score_record(score, R, B, direction, valid_keys, n0, N_cap, ukeys, counter, stream)
    ok = [fake, 8, 100, 1, fake, 3, 103, fake, fake, None]
    for i in (0, 7):
        args = list(ok)
        args[i] = None
        assert lib.bmi_score_record(*args) == INVALID_, i
    for i, values in ((1, (0, -1)), (2, (0, -1, 101)), (3, (0, 2, -2)), (5, (-1, 4)), (6, (0, -1, 102))):
        for v in values:
            args = list(ok)
            args[i] = v
            assert lib.bmi_score_record(*args) == INVALID_, (i, v)
    args = list(ok)
    args[1] = 1025
    assert lib.bmi_score_record(*args) == UNSUPPORTED
    args = list(ok)
    args[2], args[5], args[6] = 2 ** 17 + 1, 0, 2 ** 17 + 1
    assert lib.bmi_score_record(*args) == UNSUPPORTED
    # bmi_rank_quality(ukeys, positive, R, N, N_cap, rank, sorted_keys, curve, counts, aurc_sum, scratch, scratch_bytes, stream)
    need = lib.bmi_rank_scratch_bytes(8, 1000)
    ok = [fake, fake, 8, 1000, 1003] + [fake] * 6 + [need, None]
    for i in (0, 1, 5, 6, 7, 8, 9, 10):
        args = list(ok)
        args[i] = None
        assert lib.bmi_rank_quality(*args) == INVALID_, i
    for i, values in ((2, (0, -1)), (3, (0, -1, 1004)), (4, (999, 0))):
        for v in values:
            args = list(ok)
            args[i] = v
            assert lib.bmi_rank_quality(*args) == INVALID_, (i, v)
    args = list(ok)
    args[2], args[11] = 1025, 1 << 40
    assert lib.bmi_rank_quality(*args) == UNSUPPORTED
    args = list(ok)
    args[3], args[4], args[11] = 2 ** 17 + 1, 2 ** 17 + 1, 1 << 40
    assert lib.bmi_rank_quality(*args) == UNSUPPORTED
    for short in (0, need - 1):
        args = list(ok)
        args[11] = short
        assert lib.bmi_rank_quality(*args) == NOMEM, short
