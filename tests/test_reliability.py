"""-m gpu: reliability tables on the device (bmi_reliability_record / bmi_reliability_table, MCDEngine.reliability_records /
reliability_table, train.reliability.ReliabilityAnalysis) — the kernels against ``reliability_numpy`` (keys, hits, edges, integer bins and
the Brier numbers bit for bit; the NLL numbers to 1e-12 relative: the device's ``log`` and numpy's may differ in the last place, the test
prints how many records do), batch-split invariance, reproducibility, errors that write nothing, the counters, graph capture, and the
walk against FullAnalysis' own arrays."""
import ctypes as C

import numpy as np
import pytest
import torch

from bayesnn_fpga_amd import _lib
from bayesnn_fpga_amd.engine import MCDEngine
from bayesnn_fpga_amd.models.resnet18.resnet18 import ResNet18MCEarlyExit
from bayesnn_fpga_amd.synthetic import synthetic_images, synthetic_labels, synthetic_weights_
from bayesnn_fpga_amd.train import FullAnalysis, ReliabilityAnalysis
from bayesnn_fpga_amd.train.metrics import ece_hist_binary
from bayesnn_fpga_amd.train.reliability import reliability_numpy, row_names, table_metrics, width_edges
from tests.gpu_helpers import ptr, stream
from tests.helpers import build_seeded
from tests.test_reliability_host import CASES, ECE_BOUND, make_case, restated

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
PAD = 16                      # canary entries in front of and behind each buffer
SPARE = 3                     # record columns beyond N: never written
INTS = ("count", "hits", "conf_fix")
RECORDS = ("keys", "hit", "nll", "brier")
FILL = dict(keys=-7, hit=249, nll=float("nan"), brier=float("nan"), edges=float("nan"), count=-7, hits=-7, conf_fix=-7, sums=float("nan"))
DTYPES = dict(keys=torch.int32, hit=torch.uint8, nll=torch.float64, brier=torch.float64, edges=torch.float32, count=torch.int64,
              hits=torch.int64, conf_fix=torch.int64, sums=torch.float64)


def untouched(a, fill):
    return np.isnan(a) if isinstance(fill, float) else a == fill


class Buffers:
    """The record buffers [R][N + SPARE] and the table outputs, each filled with NaN / -7 / 249 and with canaries around it"""

    def __init__(self, R, N, n_bins):
        self.R, self.N, self.cap, self.n_bins = R, N, N + SPARE, n_bins
        self.size = dict(keys=R * self.cap, hit=R * self.cap, nll=R * self.cap, brier=R * self.cap, edges=R * (n_bins + 1), count=R * n_bins,
                         hits=R * n_bins, conf_fix=R * n_bins, sums=R * 2)
        self.flat = {k: torch.full((PAD + n + PAD,), FILL[k], dtype=DTYPES[k], device=DEV) for k, n in self.size.items()}
        self.counters = torch.full((2,), 100, dtype=torch.int32, device=DEV)

    def p(self, name):
        t = self.flat[name]
        return C.c_void_p(t.data_ptr() + PAD * t.element_size())

    def read(self):
        """(the arrays, whether every canary and every spare record column is as it was filled)"""
        out, intact = {}, True
        for k, t in self.flat.items():
            a = t.cpu().numpy()
            intact &= bool(untouched(a[:PAD], FILL[k]).all() and untouched(a[-PAD:], FILL[k]).all())
            a = a[PAD:-PAD]
            if k in RECORDS:
                a = a.reshape(self.R, self.cap)
                intact &= bool(untouched(a[:, self.N:], FILL[k]).all())
                a = a[:, :self.N]
            out[k] = a.reshape(self.R, -1) if k not in RECORDS else a
        out["keys"] = np.ascontiguousarray(out["keys"]).view(np.uint32)
        out["nll_sum"], out["brier_sum"] = out["sums"][:, 0].copy(), out["sums"][:, 1].copy()
        out["counters"] = (self.counters.cpu().numpy() - 100).tolist()
        return out, intact


def record(buf, p, y, cuts=None, count=True, n0=0):
    """bmi_reliability_record over the batches ``cuts`` (sizes; default: one call) -> the return codes"""
    lib, E, N, C_ = _lib.lib(), *p.shape
    rcs, off, keep = [], 0, []
    yd = torch.from_numpy(np.asarray(y).astype(np.int32)).to(DEV)
    for b in cuts or [N]:
        mean = torch.from_numpy(np.ascontiguousarray(p[:, off:off + b])).to(DEV)
        keep.append(mean)
        rcs.append(lib.bmi_reliability_record(ptr(mean), E, b, C_, ptr(yd[off:off + b].contiguous()), n0 + off, buf.cap, buf.p("keys"),
                                              buf.p("hit"), buf.p("nll"), buf.p("brier"), ptr(buf.counters) if count else None, stream()))
        off += b
    assert off == N
    torch.cuda.synchronize()
    return rcs


def table(buf, edges_in=None, scratch_bytes=None, n_bins=None):
    lib = _lib.lib()
    n_bins = buf.n_bins if n_bins is None else n_bins
    need = int(lib.bmi_reliability_scratch_bytes(buf.R, buf.N, buf.n_bins))
    assert need == buf.R * -(-buf.N // 4096) * 3 * buf.n_bins * 8
    scratch = torch.empty(need, dtype=torch.uint8, device=DEV)
    rc = lib.bmi_reliability_table(buf.p("keys"), buf.p("hit"), buf.p("nll"), buf.p("brier"), buf.R, buf.N, buf.cap, n_bins,
                                   None if edges_in is None else (C.c_float * len(edges_in))(*edges_in), buf.p("edges"), buf.p("count"),
                                   buf.p("hits"), buf.p("conf_fix"), buf.p("sums"), ptr(scratch), need if scratch_bytes is None else scratch_bytes,
                                   stream())
    torch.cuda.synchronize()
    return rc


def run(p, y, cuts=None, n_bins=15, edges_in=None):
    buf = Buffers(2 * p.shape[0], p.shape[1], n_bins)
    rcs = record(buf, p, y, cuts)
    rc = table(buf, edges_in)
    got, intact = buf.read()
    assert all(r == _lib.BMI_OK for r in rcs) and rc == _lib.BMI_OK and intact
    return got


def same_bits(a, b, names):
    return all(np.array_equal(np.ascontiguousarray(a[k]).view(np.uint8), np.ascontiguousarray(b[k]).view(np.uint8)) for k in names)


def assert_equals_restatement(got, want, what):
    """keys, hits, edges, the integer bins and the Brier numbers bit for bit; the NLL numbers to 1e-12 relative"""
    last_place = int((got["nll"].view(np.int64) != want["nll"].view(np.int64)).sum())
    print(f"{what}: NLL records whose bits differ from numpy's log: {last_place} of {got['nll'].size}")
    assert np.array_equal(got["keys"], want["keys"]) and np.array_equal(got["hit"], want["hit"])
    assert np.array_equal(got["edges"].view(np.uint32), want["edges"].view(np.uint32))
    for k in INTS:
        assert np.array_equal(got[k], want[k]), k
    assert np.array_equal(got["brier"].view(np.int64), want["brier"].view(np.int64))
    assert np.array_equal(got["brier_sum"].view(np.int64), want["brier_sum"].view(np.int64))
    np.testing.assert_allclose(got["nll"], want["nll"], rtol=1e-12, atol=0)
    np.testing.assert_allclose(got["nll_sum"], want["nll_sum"], rtol=1e-12, atol=0)
    # the device's own NLL records added in image order on the host: its sum bit for bit
    own = [sum(row.tolist(), 0.0) for row in got["nll"]]
    assert np.array_equal(np.array(own).view(np.int64), got["nll_sum"].view(np.int64))


ALL = RECORDS + ("edges",) + INTS + ("sums",)
KERNEL_CASES = CASES + [(32, 3, 65, 3, 6, 0), (4, 64, 2, 1, 8, 1.0)]


@pytest.mark.parametrize("case", KERNEL_CASES, ids=lambda c: "E{}N{}C{}".format(*c[:3]))
def test_kernels_equal_the_numpy_restatement(case):
    """Record and table kernels through the C ABI on canary-padded, NaN / -7 filled outputs; two runs give the same bits.  The last case
    has every key equal (1.0)."""
    p, y, want = restated(case)
    got = run(p, y)
    assert got["counters"] == [0, 0]
    assert_equals_restatement(got, want, case)
    assert same_bits(run(p, y), got, ALL)
    if case[5] == 1.0:
        # every edge but the first is 1.0: bin 0 = (0, 1] holds every image, the others have no width
        assert (got["keys"] == 0x3f800000).all() and (got["count"][:, 1:] == 0).all() and (got["count"][:, 0] == case[1]).all()


def test_width_binning_and_other_bin_counts():
    p, y, _ = restated(CASES[0])
    for n_bins, edges_in in ((10, width_edges(10).tolist()), (1, None), (64, None), (64, width_edges(64).tolist())):
        got = run(p, y, n_bins=n_bins, edges_in=edges_in)
        assert_equals_restatement(got, reliability_numpy(p, y, n_bins, "mass" if edges_in is None else "width"), (n_bins, edges_in is None))


def test_batch_split_invariance():
    """N = 1000 recorded as one call, as 4 x 250 and as 7 ragged calls: records and tables have identical bits"""
    p, y, want = restated(CASES[1])
    one = run(p, y)
    assert_equals_restatement(one, want, "one call")
    for cuts in ([250] * 4, [1, 63, 64, 65, 300, 7, 500]):
        assert same_bits(run(p, y, cuts), one, ALL), cuts


def test_an_error_writes_nothing():
    p, y, _ = restated(CASES[2])
    E, N, C_ = p.shape
    buf = Buffers(2 * E, N, 15)
    assert record(buf, p, y, n0=SPARE + 1) == [-22]                              # one column beyond the capacity
    need = 2 * E * 3 * 15 * 8
    assert table(buf, scratch_bytes=need - 1) == -12
    assert table(buf, n_bins=65) == -22 and table(buf, n_bins=0) == -22
    assert table(buf, edges_in=[0.0] * 8 + [0.5, 0.4] + [1.0] * 6) == -22
    got, intact = buf.read()
    assert intact and got["counters"] == [0, 0]
    for k in ALL:
        assert untouched(buf.flat[k].cpu().numpy(), FILL[k]).all(), k


def test_counters_non_finite_rows_and_bad_labels():
    p, y = make_case(3, 11, 10, 3, 9, 0)
    bad, yb = p.copy(), y.copy()
    bad[1, 2, 3] = np.nan
    bad[0, 4, :] = np.inf
    bad[2, 5, 0] = -np.inf
    yb[7], yb[8] = -1, 10
    want = reliability_numpy(bad, yb)
    got = run(bad, yb)
    assert got["counters"] == [want["nonfinite"], want["badlabel"]] == [9, 2]
    assert_equals_restatement(got, want, "invalid rows")
    for k in ("nll", "brier", "edges", "sums"):
        assert np.isfinite(got[k]).all(), k
    # without counters: the same records
    buf = Buffers(6, 11, 15)
    assert record(buf, bad, yb, count=False) == [0] and table(buf) == 0
    again, intact = buf.read()
    assert intact and again["counters"] == [0, 0] and same_bits(again, got, ALL)


def _model(kw, dtype="f16x2"):
    m = synthetic_weights_(build_seeded(ResNet18MCEarlyExit, kw), 0).to(DEV).eval()
    m.engine_dtype = dtype
    return m


KW = dict(dropout_exit=True, dropout="block", dropout_p=0.25, out_dim=10)


def test_engine_methods_and_graph_capture():
    """MCDEngine.reliability_records / reliability_table against the restatement (mass and width), the counters' two exceptions, and ONE
    torch.cuda.graph capture of record + table whose replays give the eager bits, also on new inputs."""
    eng = MCDEngine(_model(KW), DEV, max_batch=8, dtype="f16x2")
    p, y, want = restated(CASES[0])
    E, N, _ = p.shape
    rec = eng.new_reliability_records(N + 5)
    assert tuple(rec["keys"].shape) == (8, N + 5) and sum(rec[k].element_size() for k in RECORDS) == 21
    pd, yd = torch.from_numpy(p).to(DEV), torch.from_numpy(y)
    assert eng.reliability_records(pd[:, :100].contiguous(), yd[:100], rec, 0) == 100
    assert eng.reliability_records(pd[:, 100:].contiguous(), yd[100:], rec, 100) == N
    names = ("edges",) + INTS + ("nll_sum", "brier_sum")
    for binning, n_bins in (("mass", 15), ("width", 10)):
        t = eng.reliability_table(rec, N, n_bins, binning)
        w = want if binning == "mass" else reliability_numpy(p, y, n_bins, binning)
        got = {k: t[k].cpu().numpy() for k in names}
        got.update({k: rec[k][:, :N].cpu().numpy() for k in RECORDS})
        got["keys"] = np.ascontiguousarray(got["keys"]).view(np.uint32)
        assert t["n"] == N and t["count"].dtype == torch.int64 and tuple(t["edges"].shape) == (8, n_bins + 1)
        assert_equals_restatement(got, w, binning)
        m, mw = table_metrics(t), table_metrics(w)
        assert all(np.array_equal(m[k], mw[k]) for k in ("acc", "ece", "mce", "brier"))
    eager = {k: t[k].clone() for k in names}
    with pytest.raises(ValueError):
        eng.reliability_records(pd.contiguous(), yd, rec, 6)
    with pytest.raises(ValueError):
        eng.reliability_records(pd.float().contiguous(), yd, rec, 0)
    with pytest.raises(ValueError):
        eng.reliability_table(rec, N, 15, "kde")
    with pytest.raises(ValueError):
        eng.reliability_table(rec, N + 6)
    # graph capture: static inputs, the outputs allocated inside the capture
    ps, ys = pd.clone(), yd.to(DEV).clone()
    out = {}
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        eng.reliability_records(ps, ys, rec, 0)
        out.update(eng.reliability_table(rec, N, 10, "width", check=False))
    graph.replay()
    torch.cuda.synchronize()
    assert all(torch.equal(out[k], eager[k]) for k in names)
    p2, y2 = make_case(4, 250, 10, 3, 40, 0.1)
    ps.copy_(torch.from_numpy(p2))
    ys.copy_(torch.from_numpy(y2))
    graph.replay()
    torch.cuda.synchronize()
    w2 = reliability_numpy(p2, y2, 10, "width")
    assert all(np.array_equal(out[k].cpu().numpy(), w2[k]) for k in ("edges",) + INTS + ("brier_sum",))
    np.testing.assert_allclose(out["nll_sum"].cpu().numpy(), w2["nll_sum"], rtol=1e-12, atol=0)
    # the counters: a NaN row, then a bad label
    bad = pd.clone()
    bad[1, 2, 3] = float("nan")
    eng.reliability_records(bad, yd, rec, 0)
    with pytest.raises(FloatingPointError, match="4 reliability records"):       # exit 1 and the ensembles 1, 2, 3
        eng.reliability_table(rec, N)
    rec["counters"].zero_()
    yb = yd.clone()
    yb[5] = 10
    eng.reliability_records(pd, yb, rec, 0)
    with pytest.raises(ValueError, match="1 images with a label"):
        eng.reliability_table(rec, N)
    assert not any(torch.isnan(v).any() for v in eng.reliability_table(rec, N, check=False).values() if torch.is_tensor(v))


def test_reliability_analysis_against_full_analysis(tmp_path, monkeypatch):
    """The seeded ResNet-18, 2 batches of 8, T = 4: ``rows`` equal table_metrics(reliability_numpy(...)) of the preds / labels FullAnalysis
    collects on the same model, loader and seed — the keys first (the condition), then the integers and with them accuracy, ECE and MCE
    exactly, NLL and Brier to 1e-12 —, and the ECE agrees with ece_hist_binary within the host test's bound."""
    m = synthetic_weights_(build_seeded(ResNet18MCEarlyExit, KW), 0).to(DEV).eval()
    B, T, seed = 8, 4, 11
    x, y = synthetic_images(2 * B, seed=3), synthetic_labels(2 * B, 10, seed=4)
    loader = [(x[i * B:(i + 1) * B], y[i * B:(i + 1) * B]) for i in range(2)]
    fa = FullAnalysis(m, loader, gpu=0, mc_dropout=True, mc_passes=T, seed=seed, macro_batches=1, ece="hist")
    ra = ReliabilityAnalysis(m, loader, gpu=0, mc_passes=T, seed=seed)
    E, N = fa.preds.shape[0], 2 * B
    labels = fa.labels.argmax(1)
    assert ra.n == N and np.array_equal(ra.labels, labels) and np.array_equal(labels, y.numpy())
    want = reliability_numpy(fa.preds, labels)
    assert want["nonfinite"] == 0 and want["badlabel"] == 0
    keys = np.ascontiguousarray(ra.records["keys"][:, :N].cpu().numpy()).view(np.uint32)
    print(f"keys that differ from the restatement on FullAnalysis' preds: {int((keys != want['keys']).sum())}")
    assert np.array_equal(keys, want["keys"])
    assert np.array_equal(ra.table["edges"].cpu().numpy().view(np.uint32), want["edges"].view(np.uint32))
    for k in INTS:
        assert np.array_equal(ra.table[k].cpu().numpy(), want[k]), k
    mw = table_metrics(want)
    assert [r[0] for r in ra.rows] == row_names(E) == [str(e) for e in range(E)] + [f"Ensemble{e}" for e in range(E)]
    for r, row in enumerate(ra.rows):
        assert row[1:4] == (mw["acc"][r], mw["ece"][r], mw["mce"][r])
        np.testing.assert_allclose(row[4:], [mw["nll"][r], mw["brier"][r]], rtol=1e-12, atol=0)
        v = (fa.preds if r < E else fa.ensemble_preds)[r % E]
        assert abs(row[2] - ece_hist_binary(v, fa.labels)) <= ECE_BOUND
    monkeypatch.chdir(tmp_path)
    name = ra.save("t")
    lines = open(name).read().splitlines()
    assert name == "test_reliability_t.csv" and lines[0] == "Layer,Accuracy,ECE,MCE,NLL,Brier" and len(lines) == 1 + 2 * E
    assert lines[1].split(",")[0] == "0" and float(lines[-1].split(",")[2]) == ra.rows[-1][2]
