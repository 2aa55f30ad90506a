"""-m gpu: rank quality on the device (bmi_score_record, bmi_rank_quality, MCDEngine.score_records / rank_quality, RankingAnalysis) — every
output of both entries against ``score_keys_numpy`` / ``rank_quality_numpy`` bit for bit, on buffers with canaries and spare columns, at
the sizes around the two tile sizes, under every key regime, positive pattern and kind of invalid image; uneven record cuts,
reproducibility, graph capture, errors that write nothing, and the walk against ``predict_votes``' own arrays."""
import ctypes as C
import itertools

import numpy as np
import pytest
import torch

from bayesnn_fpga_amd import _lib
from bayesnn_fpga_amd.models.resnet18.resnet18 import ResNet18MCEarlyExit
from bayesnn_fpga_amd.synthetic import synthetic_images, synthetic_labels, synthetic_weights_
from bayesnn_fpga_amd.train import RankingAnalysis
from bayesnn_fpga_amd.train.ranking import (INVALID, MAX_KEY, SCORES, rank_metrics, rank_quality_numpy, risk_at_coverage, score_keys_numpy,
                                            threshold_at_coverage)
from bayesnn_fpga_amd.train.reliability import reliability_numpy, row_names
from tests.gpu_helpers import ptr, stream
from tests.helpers import build_seeded

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
PAD = 16                      # canary entries in front of and behind each buffer
SPARE = 3                     # columns beyond N: never written
WIDE = ("ukeys", "positive", "rank", "sorted_keys", "curve")        # [R][N + SPARE]
OUTPUTS = ("rank", "sorted_keys", "curve", "counts", "aurc_sum")
FILL = dict(ukeys=-7, positive=249, rank=-7, sorted_keys=-7, curve=-7, counts=-7, aurc_sum=float("nan"), counter=-7)
DTYPES = dict(ukeys=torch.int32, positive=torch.uint8, rank=torch.int32, sorted_keys=torch.int32, curve=torch.int32, counts=torch.int64,
              aurc_sum=torch.float64, counter=torch.int32)
TI, TJ = _lib.RANK_TILE_I, _lib.RANK_TILE_J
SIZES = sorted({1, 2, 63, 64, 65, TI - 1, TI, TI + 1, TJ + 1, 2 * TJ + 3, 4099})
ROWS = (1, 3, 8)
FLT_MAX = float(np.uint32(MAX_KEY).view(np.float32))
# (the keys, the positives, the invalid images) of a row: every combination occurs in test_kernels_equal_the_numpy_restatement
REGIMES = list(itertools.product(("distinct", "four levels", "equal", "extremes"), ("none", "all", "mixed"), ("none", "sprinkled", "row")))


def untouched(a, fill):
    return np.isnan(a) if isinstance(fill, float) else a == fill


class Buffers:
    """The key and positive buffers [R][N + SPARE] and the outputs of bmi_rank_quality, each filled with NaN / -7 / 249 and with canaries
    around it; the counter starts at 0 (it is added to)"""

    def __init__(self, R, N):
        self.R, self.N, self.cap = R, N, N + SPARE
        self.size = {**{k: R * self.cap for k in WIDE}, "counts": R * 3, "aurc_sum": R, "counter": 1}
        self.flat = {k: torch.full((PAD + n + PAD,), FILL[k], dtype=DTYPES[k], device=DEV) for k, n in self.size.items()}
        self.flat["counter"][PAD] = 0
        self.scratch = torch.empty(max(1, _lib.lib().bmi_rank_scratch_bytes(R, N)), dtype=torch.uint8, device=DEV)

    def p(self, name):
        t = self.flat[name]
        return C.c_void_p(t.data_ptr() + PAD * t.element_size())

    def put(self, name, a):
        """Columns 0 .. N-1 of a wide buffer from an array [R, N]"""
        a = np.ascontiguousarray(a)
        a = a.view(np.int32) if a.dtype == np.uint32 else a
        self.flat[name][PAD:PAD + self.R * self.cap].view(self.R, self.cap)[:, :self.N] = torch.from_numpy(a).to(DEV)

    def read(self):
        """(the arrays, whether every canary and every spare column is as it was filled)"""
        out, intact = {}, True
        for k, t in self.flat.items():
            a = t.cpu().numpy()
            intact &= bool(untouched(a[:PAD], FILL[k]).all() and untouched(a[-PAD:], FILL[k]).all())
            a = a[PAD:-PAD]
            if k in WIDE:
                a = a.reshape(self.R, self.cap)
                intact &= bool(untouched(a[:, self.N:], FILL[k]).all())
                a = a[:, :self.N]
            out[k] = a
        for k in ("ukeys", "sorted_keys"):
            out[k] = np.ascontiguousarray(out[k]).view(np.uint32)
        out["counts"] = out["counts"].reshape(self.R, 3)
        return out, intact

    def all_as_filled(self, names):
        return all(untouched(self.flat[k].cpu().numpy(), FILL[k]).all() for k in names)


def record(buf, scores, way, cuts, valid=None, **change):
    """bmi_score_record over the batches ``cuts`` (sizes); ``valid``: uint32 [R, N] -> the last return code"""
    lib, off, keep, rc = _lib.lib(), 0, [], _lib.BMI_OK
    vk = None
    if valid is not None:
        vk = torch.zeros(buf.R, buf.cap, dtype=torch.int32, device=DEV)
        vk[:, :buf.N] = torch.from_numpy(np.ascontiguousarray(valid).view(np.int32)).to(DEV)
    for b in cuts:
        part = torch.from_numpy(np.ascontiguousarray(scores[:, off:off + b])).to(DEV)
        keep.append(part)
        a = dict(score=ptr(part), R=buf.R, B=b, direction=way, valid_keys=ptr(vk), n0=off, N_cap=buf.cap, ukeys=buf.p("ukeys"),
                 counter=buf.p("counter"))
        a.update(change)
        rc = lib.bmi_score_record(*a.values(), stream())
        off += b
    torch.cuda.synchronize()
    return rc


def rank(buf, **change):
    """bmi_rank_quality on the buffers; ``change``: arguments replaced by name -> the return code"""
    a = dict(ukeys=buf.p("ukeys"), positive=buf.p("positive"), R=buf.R, N=buf.N, N_cap=buf.cap, **{k: buf.p(k) for k in OUTPUTS},
             scratch=ptr(buf.scratch), scratch_bytes=buf.scratch.numel())
    a.update(change)
    rc = _lib.lib().bmi_rank_quality(*a.values(), stream())
    torch.cuda.synchronize()
    return rc


def same_bits(a, b, names=OUTPUTS):
    return all(np.array_equal(np.ascontiguousarray(a[k]).view(np.uint8), np.ascontiguousarray(b[k]).view(np.uint8)) for k in names)


def assert_equals_restatement(got, ukeys, positive, N, what):
    """Every output against rank_quality_numpy, bit for bit -> the restatement"""
    want = rank_quality_numpy(ukeys, positive, N)
    for k in OUTPUTS:
        assert got[k].dtype == want[k].dtype and got[k].shape == want[k].shape, (what, k)
        differ = int((np.ascontiguousarray(got[k]).view(np.uint8) != np.ascontiguousarray(want[k]).view(np.uint8)).reshape(got[k].size, -1)
                     .any(axis=1).sum())
        if differ:
            print(f"{what}: {k}: {differ} of {got[k].size} values differ from the restatement")
        assert differ == 0, (what, k)
    return want


def cuts_of(N):
    """Uneven batches that add up to N: 1, 7, the rest"""
    cuts, left = [], N
    for b in (1, 7):
        if left > b:
            cuts.append(b)
            left -= b
    return cuts + [left]


def make_row(N, regime, rng):
    """-> (score float64 [N], positive uint8 [N], valid uint32 [N]) of one row under ``regime`` = (keys, positives, invalid images)"""
    keys, positives, invalid = regime
    if keys == "distinct":
        s = rng.permutation(N).astype(np.float64) / 8.0 + 0.125          # distinct float32 values, in no order
    elif keys == "four levels":
        s = rng.integers(0, 4, N).astype(np.float64) * 0.25             # heavy ties, across every tile border
    elif keys == "equal":
        s = np.full(N, 0.75)
    else:
        s = np.where(rng.random(N) < 0.5, 0.0, FLT_MAX)                 # the keys 0 and 0x7F7FFFFF
        s[::5] = -0.0
    pos = dict(none=np.zeros(N), all=np.ones(N), mixed=rng.random(N) < 0.3)[positives].astype(np.uint8)
    valid = np.full(N, 0x3F000000, dtype=np.uint32)
    if invalid == "sprinkled":                                           # 2 %, at least one: by the score and by valid_keys in turn
        at = rng.choice(N, max(1, N // 50), replace=False)
        s[at[0::2]] = rng.choice([np.nan, np.inf, -1.0], len(at[0::2]))
        valid[at[1::2]] = 0
    elif invalid == "row":
        s[:] = np.nan
    return s, pos, valid


CASES = [(N, R) for N in SIZES for R in ROWS]


@pytest.mark.parametrize("case", CASES, ids=lambda c: "N{}R{}".format(*c))
def test_kernels_equal_the_numpy_restatement(case):
    """Scores recorded in uneven cuts into canary-padded buffers with spare columns, then the two rank kernels: the keys, the counter and
    every output bit for bit, twice, and once more from keys recorded in one call"""
    N, R = case
    first = CASES.index(case) // len(ROWS) * sum(ROWS) + sum(r for r in ROWS if r < R)     # consecutive over the cases: every regime occurs
    rng = np.random.default_rng(first)
    rows = [make_row(N, REGIMES[(first + r) % len(REGIMES)], rng) for r in range(R)]
    score, positive, valid = (np.stack([row[i] for row in rows]) for i in range(3))
    direction = 1 if first % 2 else -1
    buf = Buffers(R, N)
    buf.put("positive", positive)
    assert record(buf, score, direction, cuts_of(N), valid) == _lib.BMI_OK and rank(buf) == _lib.BMI_OK
    got, intact = buf.read()
    assert intact
    ukeys, bad = score_keys_numpy(score, direction, valid)
    assert np.array_equal(got["ukeys"], ukeys) and got["counter"][0] == bad
    want = assert_equals_restatement(got, ukeys, positive, N, case)
    assert np.isfinite(got["aurc_sum"]).all() and (want["counts"][:, 0] == (ukeys != INVALID).sum(axis=1)).all()
    assert rank(buf) == _lib.BMI_OK
    assert same_bits(buf.read()[0], got)
    other = Buffers(R, N)
    other.put("positive", positive)
    assert record(other, score, direction, [N], valid) == _lib.BMI_OK and rank(other) == _lib.BMI_OK
    again, intact = other.read()
    assert intact and same_bits(again, got, OUTPUTS + ("ukeys", "counter"))


def test_every_regime_occurs():
    seen = set()
    for i, (N, R) in enumerate(CASES):
        first = i // len(ROWS) * sum(ROWS) + sum(r for r in ROWS if r < R)
        seen |= {(first + r) % len(REGIMES) for r in range(R)}
    assert seen == set(range(len(REGIMES)))


def test_record_without_valid_keys_and_without_a_counter():
    N, R = 130, 2
    rng = np.random.default_rng(0)
    score = rng.random((R, N))
    score[0, 5], score[1, 9], score[1, 64] = np.nan, -0.5, np.inf
    for direction in (1, -1):
        buf = Buffers(R, N)
        assert record(buf, score, direction, cuts_of(N)) == _lib.BMI_OK
        got, intact = buf.read()
        ukeys, bad = score_keys_numpy(score, direction)
        assert intact and np.array_equal(got["ukeys"], ukeys) and got["counter"][0] == bad == 3
        assert record(buf, score, direction, [N], counter=None) == _lib.BMI_OK
        got, intact = buf.read()
        assert intact and np.array_equal(got["ukeys"], ukeys) and got["counter"][0] == 3


def test_an_error_writes_nothing():
    N, R = 300, 2
    rng = np.random.default_rng(1)
    score, positive = rng.random((R, N)), (rng.random((R, N)) < 0.3).astype(np.uint8)
    buf = Buffers(R, N)
    INVALID_, UNSUPPORTED, NOMEM = -22, -95, -12
    for change in (dict(score=None), dict(ukeys=None), dict(R=0), dict(B=0), dict(direction=0), dict(direction=2), dict(n0=-1), dict(n0=4),
                   dict(N_cap=N - 1), dict(N_cap=0)):
        assert record(buf, score, 1, [N], **change) == INVALID_, change
    assert record(buf, score, 1, [N], R=1025) == UNSUPPORTED
    assert buf.read()[1] and buf.all_as_filled(("ukeys",)) and buf.read()[0]["counter"][0] == 0
    buf.put("positive", positive)
    assert record(buf, score, 1, [N]) == _lib.BMI_OK
    for name in ("ukeys", "positive", "scratch") + OUTPUTS:
        assert rank(buf, **{name: None}) == INVALID_, name
    for change in (dict(R=0), dict(N=0), dict(N=buf.cap + 1), dict(N_cap=N - 1)):
        assert rank(buf, **change) == INVALID_, change
    for change in (dict(R=1025, scratch_bytes=1 << 40), dict(N=2 ** 17 + 1, N_cap=2 ** 17 + 1, scratch_bytes=1 << 40)):
        assert rank(buf, **change) == UNSUPPORTED, change
    assert rank(buf, scratch_bytes=buf.scratch.numel() - 1) == NOMEM
    assert buf.read()[1] and buf.all_as_filled(OUTPUTS)
    assert rank(buf) == _lib.BMI_OK and not buf.all_as_filled(OUTPUTS)


KW = dict(dropout_exit=True, dropout="block", dropout_p=0.25, out_dim=10)


def _model():
    m = synthetic_weights_(build_seeded(ResNet18MCEarlyExit, KW), 0).to(DEV).eval()
    m.engine_dtype = "f16x2"
    return m


def test_engine_methods_and_graph_capture():
    """MCDEngine.score_records / rank_quality against the restatements, their argument errors, and ONE torch.cuda.graph capture of the
    record call and the rank call whose replay gives the eager bits, also on new scores"""
    eng = _model().engine(torch.device(DEV), max_batch=8, dtype="f16x2")
    R, N, cap = 8, TI + 37, TI + 42
    rng = np.random.default_rng(2)
    score, positive = rng.integers(0, 50, (R, N)) / 64.0, (rng.random((R, cap)) < 0.4).astype(np.uint8)
    score[3, 11] = np.nan
    valid = np.full((R, cap), 0x3F000000, dtype=np.uint32)
    valid[2, 7] = 0
    sd, pd, vd = torch.from_numpy(score).to(DEV), torch.from_numpy(positive).to(DEV), torch.from_numpy(valid.view(np.int32)).to(DEV)
    rec = eng.new_score_records(cap, R)
    assert rec["ukeys"].dtype == torch.int32 and (rec["ukeys"] == -1).all() and rec["counter"].tolist() == [0]
    assert eng.score_records(sd[:, :100].contiguous(), rec, 0, -1, valid=vd) == 100
    assert eng.score_records(sd[:, 100:].contiguous(), rec, 100, -1, valid=vd) == N
    ukeys, bad = score_keys_numpy(score, -1, valid[:, :N])
    assert np.array_equal(rec["ukeys"][:, :N].cpu().numpy().view(np.uint32), ukeys) and rec["counter"].tolist() == [bad] == [1]
    assert (rec["ukeys"][:, N:] == -1).all()

    def check(out, ukeys):
        got = {k: out[k][:, :N].contiguous().cpu().numpy() if k in WIDE else out[k].cpu().numpy() for k in OUTPUTS}
        got["sorted_keys"] = got["sorted_keys"].view(np.uint32)
        assert out["n"] == N and all((out[k][:, N:] == 0).all() for k in ("rank", "sorted_keys", "curve"))
        return assert_equals_restatement(got, ukeys, positive[:, :N], N, "engine")

    eager = eng.rank_quality(rec["ukeys"], pd, N)
    check(eager, ukeys)
    for bad_call in (lambda: eng.rank_quality(rec["ukeys"], pd, 0), lambda: eng.rank_quality(rec["ukeys"], pd, cap + 1),
                     lambda: eng.rank_quality(rec["ukeys"], pd[:, :N].contiguous(), N), lambda: eng.score_records(sd, rec, 0, 0),
                     lambda: eng.score_records(sd, rec, 6, 1), lambda: eng.score_records(sd, rec, 0, 1, valid=vd[:, :N].contiguous()),
                     lambda: eng.score_records(sd.float(), rec, 0, 1), lambda: eng.new_score_records(0, 1)):
        with pytest.raises(ValueError):
            bad_call()
    # graph capture on a side stream (torch.cuda.graph's own): static inputs, the outputs allocated inside the capture
    ss = sd.clone()
    out = {}
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        eng.score_records(ss, rec, 0, -1, valid=vd)
        out.update(eng.rank_quality(rec["ukeys"], pd, N))
    graph.replay()
    torch.cuda.synchronize()
    assert all(torch.equal(out[k], eager[k]) for k in OUTPUTS)
    score2 = rng.random((R, N))
    ss.copy_(torch.from_numpy(score2))
    graph.replay()
    torch.cuda.synchronize()
    check(out, score_keys_numpy(score2, -1, valid[:, :N])[0])


def test_ranking_analysis_against_the_walks_own_arrays(tmp_path, monkeypatch):
    """The seeded ResNet-18, three batches of 8, 5 and 3 images, T = 4: every table equals rank_quality_numpy fed from predict_votes' arrays
    of the same walk; again with 8 noise images behind them; the thresholds equal the host-sorted scores"""
    m = _model()
    T, seed = 4, 11
    x, y = synthetic_images(16, seed=3), synthetic_labels(16, 10, seed=4)
    loader = [(x[a:b], y[a:b]) for a, b in ((0, 8), (8, 13), (13, 16))]
    noise = [(synthetic_images(8, seed=99),)]
    scores = tuple(SCORES)
    plain = RankingAnalysis(m, loader, gpu=0, mc_passes=T, seed=seed, scores=scores)
    ra = RankingAnalysis(m, loader, gpu=0, mc_passes=T, seed=seed, scores=scores, ood_loader=noise)
    # the same walk by hand: predict_votes per batch under seed + k
    eng = m.engine(torch.device(DEV), max_batch=8, dtype="f16x2")
    E = eng.n_exits
    R, N, M = 2 * E, 16, 8
    parts = [eng.predict_votes(b[0].to(DEV), T, seed + k) for k, b in enumerate(loader + noise)]
    mean = np.concatenate([p["mean"].cpu().numpy() for p in parts], axis=1)
    rel = reliability_numpy(mean, np.concatenate([y.numpy(), np.zeros(M, dtype=np.int64)]))
    host = {s: np.concatenate([np.concatenate([p[s].cpu().numpy(), p["ens_" + s].cpu().numpy()]) for p in parts], axis=1)
            for s in scores if s != "confidence"}
    host["confidence"] = rel["keys"].view(np.float32).astype(np.float64)
    assert plain.n == ra.n == N and ra.n_ood == M and plain.n_ood == 0 and np.array_equal(ra.labels, y.numpy()) and plain.ood_rows == []
    assert [r[0] for r in plain.rows[::len(scores)]] == row_names(E) and len(plain.rows) == R * len(scores) and str(plain.rows) == str(ra.rows)
    positive = 1 - rel["hit"][:, :N]
    for s in scores:
        for an, table, ukeys, pos, n in ((plain, plain.tables[s], score_keys_numpy(host[s][:, :N], SCORES[s], rel["keys"][:, :N])[0], positive, N),
                                        (ra, ra.ood_tables[s], score_keys_numpy(host[s], SCORES[s])[0],
                                         np.concatenate([np.zeros((R, N)), np.ones((R, M))], axis=1).astype(np.uint8), N + M)):
            got = {k: table[k][:, :n].contiguous().cpu().numpy() if k in WIDE else table[k].cpu().numpy() for k in OUTPUTS}
            got["sorted_keys"] = got["sorted_keys"].view(np.uint32)
            want = assert_equals_restatement(got, ukeys, pos, n, (s, n))
            assert (want["counts"][:, 0] == n).all()
        wm = rank_metrics(rank_quality_numpy(score_keys_numpy(host[s][:, :N], SCORES[s])[0], positive, N))
        for k in ("auroc", "aurc", "eaurc"):
            assert np.array_equal(plain.metrics[s][k], wm[k], equal_nan=True), (s, k)
        # the threshold at coverage c is the host-sorted score at the same k (float32: what the keys hold)
        f32 = host[s][:, :N].astype(np.float32)
        srt = np.sort(f32, axis=1) if SCORES[s] > 0 else -np.sort(-f32, axis=1)
        for c, k in ((1.0 / N, 1), (0.5, 8), (0.8, 13), (1.0, N)):
            assert np.array_equal(threshold_at_coverage(plain.tables[s], c, SCORES[s]), srt[:, k - 1]), (s, c)
        assert np.array_equal(plain.metrics[s]["risk80"], risk_at_coverage(plain.tables[s], 0.8))
    assert np.allclose(ra.ape[0], host["pred_entropy"][:, :N].mean(axis=1), rtol=1e-12) and np.allclose(ra.ape[1], host["pred_entropy"][:, N:].mean(axis=1), rtol=1e-12)
    assert len(ra.ood_rows) == R * len(scores) and all(len(r) == 5 and 0.0 <= r[2] <= 1.0 for r in ra.ood_rows)
    print("walk: AUROC (errors) " + ", ".join(f"{r[0]}/{r[1]}={r[2]:.3f}" for r in plain.rows[-len(scores):]))
    print("walk: AUROC (noise)  " + ", ".join(f"{r[0]}/{r[1]}={r[2]:.3f}" for r in ra.ood_rows[-len(scores):]))
    monkeypatch.chdir(tmp_path)
    lines = open(plain.save("p")).read().splitlines()
    assert lines[0] == "Layer,Score,AUROC,AURC,E-AURC,Risk@0.8" and lines[1:] == [",".join(str(v) for v in r) for r in plain.rows]
    lines = open(ra.save("o")).read().splitlines()
    assert lines[0].endswith(",AUROC_OOD") and len(lines) == 1 + R * len(scores) and len(lines[1].split(",")) == 7
