"""-m gpu: classwise reliability tables on the device (bmi_classwise_record / bmi_classwise_table, MCDEngine.classwise_records /
classwise_table, ReliabilityAnalysis(classwise=True)) — the kernels against ``classwise_numpy`` bit for bit (keys, label records, edges and
the three integer tables: there is no floating-point sum), batch-split invariance, errors that write nothing, the counters, graph capture,
and the walk against FullAnalysis' own arrays."""
import ctypes as C

import numpy as np
import pytest
import torch

from bayesnn_fpga_amd import _lib
from bayesnn_fpga_amd.engine import MCDEngine
from bayesnn_fpga_amd.models.resnet18.resnet18 import ResNet18MCEarlyExit
from bayesnn_fpga_amd.synthetic import synthetic_images, synthetic_labels, synthetic_weights_
from bayesnn_fpga_amd.train import FullAnalysis, ReliabilityAnalysis
from bayesnn_fpga_amd.train.reliability import classwise_metrics, classwise_numpy, reliability_numpy
from tests.gpu_helpers import ptr, stream
from tests.helpers import build_seeded
from tests.test_classwise_host import CASES, IDS, THRESHOLD_EDGES, restated
from tests.test_reliability_host import make_case

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
PAD = 16                      # canary entries in front of and behind each buffer
SPARE = 3                     # record columns beyond N: never written
TABLE = ("edges", "count", "hits", "conf_fix", "valid")
FILL = dict(pkeys=-7, labels=-7, edges=float("nan"), count=-7, hits=-7, conf_fix=-7, valid=-7)
DTYPES = dict(pkeys=torch.int32, labels=torch.int32, edges=torch.float32, count=torch.int64, hits=torch.int64, conf_fix=torch.int64,
              valid=torch.int64)
# (binning, n_bins, fixed edges): equal width, by mass, the thresholded fixed edges, and the largest bin count of both
CONFIGS = [("width", 15, None), ("mass", 15, None), ("edges", 5, THRESHOLD_EDGES), ("width", 64, None), ("mass", 64, None)]


def untouched(a, fill):
    return np.isnan(a) if isinstance(fill, float) else a == fill


def padded(name, n):
    return torch.full((PAD + n + PAD,), FILL[name], dtype=DTYPES[name], device=DEV)


def inner(t, name):
    """(the buffer without its canaries, whether they are as they were filled)"""
    a = t.cpu().numpy()
    return a[PAD:-PAD], bool(untouched(a[:PAD], FILL[name]).all() and untouched(a[-PAD:], FILL[name]).all())


def at(t):
    return C.c_void_p(t.data_ptr() + PAD * t.element_size())


class Records:
    """pkeys [R][C][N + SPARE] and labels [N + SPARE], filled with -7 and with canaries around them"""

    def __init__(self, R, Cd, N):
        self.R, self.C, self.N, self.cap = R, Cd, N, N + SPARE
        self.pkeys, self.labels = padded("pkeys", R * Cd * self.cap), padded("labels", self.cap)
        self.counters = torch.full((2,), 100, dtype=torch.int32, device=DEV)

    def read(self):
        k, ok1 = inner(self.pkeys, "pkeys")
        l, ok2 = inner(self.labels, "labels")
        k = k.reshape(self.R, self.C, self.cap)
        intact = ok1 and ok2 and bool((k[:, :, self.N:] == FILL["pkeys"]).all() and (l[self.N:] == FILL["labels"]).all())
        return dict(pkeys=np.ascontiguousarray(k[:, :, :self.N]).view(np.uint32), labels=l[:self.N].copy(),
                    counters=(self.counters.cpu().numpy() - 100).tolist()), intact


def record(rec, p, y, cuts=None, count=True, n0=0):
    """bmi_classwise_record over the batches ``cuts`` (sizes; default: one call) -> the return codes"""
    lib, (E, N, C_) = _lib.lib(), p.shape
    rcs, off, keep = [], 0, []
    yd = torch.from_numpy(np.asarray(y).astype(np.int32)).to(DEV)
    for b in cuts or [N]:
        mean = torch.from_numpy(np.ascontiguousarray(p[:, off:off + b])).to(DEV)
        keep.append(mean)
        rcs.append(lib.bmi_classwise_record(ptr(mean), E, b, C_, ptr(yd[off:off + b].contiguous()), n0 + off, rec.cap, at(rec.pkeys),
                                            at(rec.labels), ptr(rec.counters) if count else None, stream()))
        off += b
    assert off == N
    torch.cuda.synchronize()
    return rcs


def table(rec, n_bins, edges_in=None, out=None, n_bins_arg=None):
    """bmi_classwise_table into fresh canary-padded outputs (or ``out``) -> (rc, the arrays, canaries intact, the buffers)"""
    L = rec.R * rec.C
    size = dict(edges=L * (n_bins + 1), count=L * n_bins, hits=L * n_bins, conf_fix=L * n_bins, valid=rec.R)
    out = out or {k: padded(k, n) for k, n in size.items()}
    rc = _lib.lib().bmi_classwise_table(at(rec.pkeys), at(rec.labels), rec.R, rec.C, rec.N, rec.cap, n_bins if n_bins_arg is None else n_bins_arg,
                                        None if edges_in is None else (C.c_float * len(edges_in))(*edges_in), at(out["edges"]), at(out["count"]),
                                        at(out["hits"]), at(out["conf_fix"]), at(out["valid"]), stream())
    torch.cuda.synchronize()
    got, intact = {}, True
    for k in TABLE:
        a, ok = inner(out[k], k)
        intact &= ok
        got[k] = a.reshape((rec.R,) if k == "valid" else (rec.R, rec.C, -1))
    return rc, got, intact, out


def run(p, y, configs, cuts=None):
    """Records once, one table per config -> (the records, [table per config])"""
    rec = Records(2 * p.shape[0], p.shape[2], p.shape[1])
    rcs = record(rec, p, y, cuts)
    got, intact = rec.read()
    assert all(r == _lib.BMI_OK for r in rcs) and intact
    tables = []
    for binning, n_bins, edges in configs:
        rc, t, ok, _ = table(rec, n_bins, edges if binning == "edges" else (None if binning == "mass" else np_width(n_bins)))
        assert rc == _lib.BMI_OK and ok, (binning, n_bins)
        tables.append(t)
    again, intact = rec.read()
    assert intact and same_bits(again, got, ("pkeys", "labels"))                 # the table call writes no record
    return got, tables


def np_width(n_bins):
    return [float(np.float32(i) / np.float32(n_bins)) for i in range(n_bins + 1)]


def same_bits(a, b, names):
    return all(np.array_equal(np.ascontiguousarray(a[k]).view(np.uint8), np.ascontiguousarray(b[k]).view(np.uint8)) for k in names)


def assert_equals_restatement(got, t, want, what):
    assert np.array_equal(got["pkeys"], want["pkeys"]), what
    assert np.array_equal(got["labels"], want["labels"]), what
    assert np.array_equal(t["edges"].view(np.uint32), want["edges"].view(np.uint32)), what
    for k in ("count", "hits", "conf_fix", "valid"):
        assert np.array_equal(t[k], want[k]), (what, k)


@pytest.mark.parametrize("case", CASES, **IDS)
def test_kernels_equal_the_numpy_restatement(case):
    """Record and table kernels through the C ABI on canary-padded, -7 / NaN filled outputs: width, mass and fixed edges, 15 and 64 bins"""
    p, y = restated(case)[:2]
    got, tables = run(p, y, CONFIGS)
    assert got["counters"] == [0, 0]
    for (binning, n_bins, edges), t in zip(CONFIGS, tables):
        assert_equals_restatement(got, t, restated(case, n_bins, binning, edges)[2], (case, binning, n_bins))
    top = reliability_numpy(p, y)                                                # the arg-max key is the top-label record's
    pred = np.maximum(np.concatenate([p, np.cumsum(p, 0) / np.arange(1, len(p) + 1.0)[:, None, None]]), 1e-256).argmax(2)
    assert np.array_equal(np.take_along_axis(got["pkeys"], pred[:, None, :], axis=1)[:, 0], top["keys"])


def test_batch_split_invariance():
    """Cuts [1, 63, 64, rest] of 250 and of 4097 images, and one call per image of 37: records and tables byte for byte the single call's"""
    configs = CONFIGS[:3]
    for case, cuts in ((CASES[4], [1, 63, 64, 122]), (CASES[5], [1, 63, 64, 3969]), (CASES[1], [1] * 37)):
        p, y = restated(case)[:2]
        one, tables = run(p, y, configs)
        cut, cut_tables = run(p, y, configs, cuts)
        assert same_bits(cut, one, ("pkeys", "labels")) and cut["counters"] == one["counters"] == [0, 0], case
        for a, b in zip(cut_tables, tables):
            assert same_bits(a, b, TABLE), case


def test_an_error_writes_nothing():
    p, y = restated(CASES[1])[:2]
    E, N, C_ = p.shape
    rec = Records(2 * E, C_, N)
    assert record(rec, p, y, n0=SPARE + 1) == [-22]                              # one column beyond the capacity
    got, intact = rec.read()
    assert intact and got["counters"] == [0, 0] and (got["pkeys"].view(np.int32) == -7).all() and (got["labels"] == -7).all()
    out = None
    for kw in (dict(n_bins_arg=65), dict(n_bins_arg=0), dict(edges_in=[0.0] * 8 + [0.5, 0.4] + [1.0] * 6),
               dict(edges_in=[0.0] * 15 + [float("nan")])):
        rc, _, intact, out = table(rec, 15, out=out, **kw)
        assert rc == -22 and intact, kw
        for k in TABLE:
            assert untouched(out[k].cpu().numpy(), FILL[k]).all(), (kw, k)
    big = Records(66, 1, 2)                                                      # R > 64: refused before any launch
    rc, _, intact, out = table(big, 15)
    assert rc == -95 and intact and all(untouched(out[k].cpu().numpy(), FILL[k]).all() for k in TABLE)


def test_counters_non_finite_rows_and_bad_labels():
    p, y = make_case(3, 11, 10, 3, 9, 0)
    bad, yb = p.copy(), y.copy()
    bad[1, 2, 3] = np.nan
    bad[0, 4, :] = np.inf
    bad[2, 5, 0] = -np.inf
    yb[7], yb[8] = -1, 10
    configs = [("width", 15, None), ("mass", 4, None)]
    got, tables = run(bad, yb, configs)
    for (binning, n_bins, _), t in zip(configs, tables):
        want = classwise_numpy(bad, yb, n_bins, binning)
        assert got["counters"] == [want["nonfinite"], want["badlabel"]] == [9, 2]
        assert_equals_restatement(got, t, want, binning)
        assert np.isfinite(t["edges"]).all()
    assert tables[1]["edges"][5, 0, 3] == 1.0                                    # an edge selected among the INVALID keys
    # without counters: the same records
    rec = Records(6, 10, 11)
    assert record(rec, bad, yb, count=False) == [0]
    again, intact = rec.read()
    assert intact and again["counters"] == [0, 0] and same_bits(again, got, ("pkeys", "labels"))


def _model(kw, dtype="f16x2"):
    m = synthetic_weights_(build_seeded(ResNet18MCEarlyExit, kw), 0).to(DEV).eval()
    m.engine_dtype = dtype
    return m


KW = dict(dropout_exit=True, dropout="block", dropout_p=0.25, out_dim=10)
NAMES = ("edges", "count", "hits", "conf_fix", "valid")


def test_engine_methods_and_graph_capture():
    """MCDEngine.new_classwise_records / classwise_records / classwise_table against the restatement, the argument checks and the
    counters' two exceptions, and ONE torch.cuda.graph capture of record + table whose replays give the eager bits, also on new inputs."""
    eng = MCDEngine(_model(KW), DEV, max_batch=8, dtype="f16x2")
    p, y = make_case(4, 250, 10, 3, 0, 0)
    E, N, Cd = p.shape
    rec = eng.new_classwise_records(N + 5)
    assert tuple(rec["pkeys"].shape) == (8, 10, N + 5) and rec["pkeys"].dtype == torch.int32 and bool((rec["pkeys"] == -1).all())
    assert tuple(rec["labels"].shape) == (N + 5,) and bool((rec["labels"] == -1).all()) and rec["counters"].tolist() == [0, 0]
    assert tuple(eng.new_classwise_records(3, n_exits=2, out_dim=7)["pkeys"].shape) == (4, 7, 3)
    pd, yd = torch.from_numpy(p).to(DEV), torch.from_numpy(y)
    assert eng.classwise_records(pd[:, :100].contiguous(), yd[:100], rec, 0) == 100
    assert eng.classwise_records(pd[:, 100:].contiguous(), yd[100:], rec, 100) == N
    for binning, n_bins, edges in (("width", 15, None), ("mass", 10, None), ("edges", None, THRESHOLD_EDGES)):
        t = eng.classwise_table(rec, N, **({} if n_bins is None else dict(n_bins=n_bins)), binning=binning, edges=edges)
        w = classwise_numpy(p, y, n_bins or 15, binning, edges)
        nb = w["count"].shape[-1]
        assert t["n"] == N and t["count"].dtype == torch.int64 and tuple(t["edges"].shape) == (8, 10, nb + 1)
        assert np.array_equal(np.ascontiguousarray(rec["pkeys"][:, :, :N].cpu().numpy()).view(np.uint32), w["pkeys"])
        assert np.array_equal(rec["labels"][:N].cpu().numpy(), w["labels"])
        assert all(np.array_equal(t[k].cpu().numpy(), w[k]) for k in NAMES), binning
        m, mw = classwise_metrics(t), classwise_metrics(w)
        assert all(np.array_equal(m[k], mw[k]) for k in mw)
    assert np.array_equal(eng.classwise_table(rec, N)["count"].cpu().numpy(), classwise_numpy(p, y)["count"])     # the default: 15 by width
    eager = {k: v.clone() for k, v in eng.classwise_table(rec, N, 10, "mass").items() if torch.is_tensor(v)}
    with pytest.raises(ValueError):
        eng.classwise_records(pd.contiguous(), yd, rec, 6)
    with pytest.raises(ValueError):
        eng.classwise_records(pd.float().contiguous(), yd, rec, 0)
    with pytest.raises(ValueError):
        eng.classwise_records(pd[:, :, :7].contiguous(), yd, rec, 0)
    for bad in (dict(binning="kde"), dict(n=N + 6), dict(n_bins=65), dict(n_bins=0), dict(binning="edges"),
                dict(binning="edges", edges=[0.0, 0.5, 0.4, 1.0])):
        with pytest.raises(ValueError):
            eng.classwise_table(rec, **{"n": N, **bad})
    # graph capture: static inputs, the outputs allocated inside the capture
    ps, ys = pd.clone(), yd.to(DEV).clone()
    out = {}
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        eng.classwise_records(ps, ys, rec, 0)
        out.update(eng.classwise_table(rec, N, 10, "mass", check=False))
    graph.replay()
    torch.cuda.synchronize()
    assert all(torch.equal(out[k], eager[k]) for k in NAMES)
    p2, y2 = make_case(4, 250, 10, 3, 40, 0.1)
    ps.copy_(torch.from_numpy(p2))
    ys.copy_(torch.from_numpy(y2))
    graph.replay()
    torch.cuda.synchronize()
    w2 = classwise_numpy(p2, y2, 10, "mass")
    assert all(np.array_equal(out[k].cpu().numpy(), w2[k]) for k in NAMES)
    # the counters: a NaN row, then a bad label
    bad = pd.clone()
    bad[1, 2, 3] = float("nan")
    eng.classwise_records(bad, yd, rec, 0)
    with pytest.raises(FloatingPointError, match="4 classwise records"):         # exit 1 and the ensembles 1, 2, 3
        eng.classwise_table(rec, N)
    rec["counters"].zero_()
    yb = yd.clone()
    yb[5] = 10
    eng.classwise_records(pd, yb, rec, 0)
    with pytest.raises(ValueError, match="1 images with a label"):
        eng.classwise_table(rec, N)
    t = eng.classwise_table(rec, N, check=False)
    assert t["valid"].tolist() == [N - 1] * 8 and not torch.isnan(t["edges"]).any()


def test_reliability_analysis_classwise_against_full_analysis(tmp_path, monkeypatch):
    """The seeded ResNet-18, 2 batches of 8, T = 4: the classwise table equals classwise_numpy of the preds / labels FullAnalysis collects
    on the same model, loader and seed, bit for bit; with default arguments rows and the CSV header are the old ones."""
    m = synthetic_weights_(build_seeded(ResNet18MCEarlyExit, KW), 0).to(DEV).eval()
    B, T, seed = 8, 4, 11
    x, y = synthetic_images(2 * B, seed=3), synthetic_labels(2 * B, 10, seed=4)
    loader = [(x[i * B:(i + 1) * B], y[i * B:(i + 1) * B]) for i in range(2)]
    fa = FullAnalysis(m, loader, gpu=0, mc_dropout=True, mc_passes=T, seed=seed, macro_batches=1, ece="hist")
    plain = ReliabilityAnalysis(m, loader, gpu=0, mc_passes=T, seed=seed)
    ra = ReliabilityAnalysis(m, loader, gpu=0, mc_passes=T, seed=seed, classwise=True)
    both = ReliabilityAnalysis(m, loader, gpu=0, mc_passes=T, seed=seed, kde=True, classwise=True, classwise_bins=5, classwise_binning="mass")
    E, N = fa.preds.shape[0], 2 * B
    labels = fa.labels.argmax(1)
    for a, nb, binning in ((ra, 15, "width"), (both, 5, "mass")):
        want = classwise_numpy(fa.preds, labels, nb, binning)
        assert want["nonfinite"] == 0 and want["badlabel"] == 0
        keys = np.ascontiguousarray(a.classwise_records["pkeys"][:, :, :N].cpu().numpy()).view(np.uint32)
        print(f"classwise keys that differ from the restatement on FullAnalysis' preds: {int((keys != want['pkeys']).sum())}")
        assert np.array_equal(keys, want["pkeys"])
        assert all(np.array_equal(a.classwise[k].cpu().numpy(), want[k]) for k in NAMES)
        mw = classwise_metrics(want)
        assert np.array_equal(a.metrics["cw_ece"], mw["cw_ece"]) and np.array_equal(a.metrics["cw_ece_per_class"], mw["cw_ece_per_class"])
        assert [row[-1] for row in a.rows] == [float(v) for v in mw["cw_ece"]]
    assert plain.classwise is False and "cw_ece" not in plain.metrics and not hasattr(plain, "classwise_records")
    assert [len(r) for r in plain.rows] == [6] * (2 * E) and [len(r) for r in ra.rows] == [7] * (2 * E) and [len(r) for r in both.rows] == [8] * (2 * E)
    assert [r[:6] for r in ra.rows] == plain.rows and [r[:6] for r in both.rows] == plain.rows
    monkeypatch.chdir(tmp_path)
    heads = [open(a.save("t")).read().splitlines() for a in (plain, ra, both)]
    assert heads[0][0] == "Layer,Accuracy,ECE,MCE,NLL,Brier" and heads[1][0] == "Layer,Accuracy,ECE,MCE,NLL,Brier,CW_ECE"
    assert heads[2][0] == "Layer,Accuracy,ECE,MCE,NLL,Brier,ECE_KDE,CW_ECE" and all(len(h) == 1 + 2 * E for h in heads)
    assert float(heads[1][-1].split(",")[6]) == ra.rows[-1][6]
