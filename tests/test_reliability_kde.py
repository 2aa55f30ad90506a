"""-m gpu: the KDE-ECE on the device (bmi_reliability_kde, MCDEngine.reliability_kde, ReliabilityAnalysis(kde=True)) — every output of the
three kernels against ``reliability_kde_numpy`` bit for bit (the contract uses no library function) on records written by
bmi_reliability_record in uneven cuts, canaries and spare columns, the host file's special cases, invalid images, reproducibility, graph
capture, errors that write nothing, and the walk against FullAnalysis' own arrays."""
import ctypes as C

import numpy as np
import pytest
import torch

from bayesnn_fpga_amd import _lib
from bayesnn_fpga_amd.engine import MCDEngine
from bayesnn_fpga_amd.models.resnet18.resnet18 import ResNet18MCEarlyExit
from bayesnn_fpga_amd.synthetic import synthetic_images, synthetic_labels, synthetic_weights_
from bayesnn_fpga_amd.train import FullAnalysis, ReliabilityAnalysis
from bayesnn_fpga_amd.train.metrics import ece_kde_binary
from bayesnn_fpga_amd.train.reliability import kde_bw_scale, reliability_kde_numpy, reliability_numpy, row_names
from tests.gpu_helpers import ptr, stream
from tests.helpers import build_seeded
from tests.test_reliability_kde_host import DEGENERATE, DIRECT_BOUND, make_probs, records_from, two_clusters

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
PAD = 16                      # canary entries in front of and behind each buffer
SPARE = 3                     # record columns beyond N: never written
RECORDS = ("keys", "hit", "nll", "brier")
OUTPUTS = ("ece_kde", "bw", "sd", "n_data", "n_hit", "degenerate", "density")
FILL = dict(keys=-7, hit=249, nll=float("nan"), brier=float("nan"), ece_kde=float("nan"), bw=float("nan"), sd=float("nan"), n_data=-7, n_hit=-7,
            degenerate=-7, density=float("nan"))
DTYPES = dict(keys=torch.int32, hit=torch.uint8, nll=torch.float64, brier=torch.float64, ece_kde=torch.float64, bw=torch.float64,
              sd=torch.float64, n_data=torch.int64, n_hit=torch.int64, degenerate=torch.int32, density=torch.float64)


def untouched(a, fill):
    return np.isnan(a) if isinstance(fill, float) else a == fill


class Buffers:
    """The record buffers [R][N + SPARE] and the outputs of bmi_reliability_kde, each filled with NaN / -7 / 249 and with canaries around it"""

    def __init__(self, R, N, G):
        self.R, self.N, self.cap, self.G = R, N, N + SPARE, G
        self.size = dict(keys=R * self.cap, hit=R * self.cap, nll=R * self.cap, brier=R * self.cap, ece_kde=R, bw=R, sd=R, n_data=R, n_hit=R,
                         degenerate=R, density=R * 2 * G)
        self.flat = {k: torch.full((PAD + n + PAD,), FILL[k], dtype=DTYPES[k], device=DEV) for k, n in self.size.items()}

    def p(self, name):
        t = self.flat[name]
        return C.c_void_p(t.data_ptr() + PAD * t.element_size())

    def put(self, keys, hit):
        """Records given as arrays [R, N] (uint32 keys, uint8 hit bits) instead of by the record kernel"""
        for name, a in (("keys", np.ascontiguousarray(keys).view(np.int32)), ("hit", np.asarray(hit, dtype=np.uint8))):
            self.flat[name][PAD:PAD + self.R * self.cap].view(self.R, self.cap)[:, :self.N] = torch.from_numpy(a).to(DEV)

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
            out[k] = a
        out["keys"] = np.ascontiguousarray(out["keys"]).view(np.uint32)
        out["density"] = out["density"].reshape(self.R, 2, self.G)
        return out, intact

    def all_as_filled(self, names):
        return all(untouched(self.flat[k].cpu().numpy(), FILL[k]).all() for k in names)


def record(buf, p, y, cuts):
    """bmi_reliability_record over the batches ``cuts`` (sizes)"""
    lib, E, N, C_ = _lib.lib(), *p.shape
    off, keep = 0, []
    yd = torch.from_numpy(np.asarray(y).astype(np.int32)).to(DEV)
    for b in cuts:
        mean = torch.from_numpy(np.ascontiguousarray(p[:, off:off + b])).to(DEV)
        keep.append(mean)
        assert lib.bmi_reliability_record(ptr(mean), E, b, C_, ptr(yd[off:off + b].contiguous()), off, buf.cap, buf.p("keys"), buf.p("hit"),
                                          buf.p("nll"), buf.p("brier"), None, stream()) == _lib.BMI_OK
        off += b
    assert off == N
    torch.cuda.synchronize()


def kde(buf, order=1, bw_scale=None, **change):
    """bmi_reliability_kde on the buffers; ``change``: arguments replaced by name -> the return code"""
    a = dict(keys=buf.p("keys"), hit=buf.p("hit"), R=buf.R, N=buf.N, N_cap=buf.cap, G=buf.G, order=order,
             bw_scale=kde_bw_scale(buf.N) if bw_scale is None else bw_scale, **{k: buf.p(k) for k in OUTPUTS})
    a.update(change)
    rc = _lib.lib().bmi_reliability_kde(*a.values(), stream())
    torch.cuda.synchronize()
    return rc


def same_bits(a, b, names=OUTPUTS):
    return all(np.array_equal(np.ascontiguousarray(a[k]).view(np.uint8), np.ascontiguousarray(b[k]).view(np.uint8)) for k in names)


def assert_equals_restatement(got, N, G, what, order=1, bw_scale=None):
    """Every output against reliability_kde_numpy of the device's own records, bit for bit -> the restatement"""
    want = reliability_kde_numpy(got["keys"], got["hit"], N, G, order, bw_scale)
    for k in OUTPUTS:
        assert got[k].dtype == want[k].dtype and got[k].shape == want[k].shape, (what, k)
        differ = int((np.ascontiguousarray(got[k]).view(np.uint8) != np.ascontiguousarray(want[k]).view(np.uint8)).reshape(got[k].size, -1)
                     .any(axis=1).sum())
        if differ:
            print(f"{what}: {k}: {differ} of {got[k].size} values differ from the restatement")
        assert differ == 0, (what, k)
    return want


def cuts_of(N):
    """Uneven batches that add up to N"""
    cuts, left = [], N
    for b in (1, 62, 65, 172, 300):
        if left > b:
            cuts.append(b)
            left -= b
    return cuts + [left]


def run_records(keys, hit, G, order=1, bw_scale=None):
    """The call on records given as arrays -> (outputs, restatement)"""
    R, N = keys.shape
    buf = Buffers(R, N, G)
    buf.put(keys, hit)
    assert kde(buf, order, bw_scale) == _lib.BMI_OK
    got, intact = buf.read()
    assert intact
    got["keys"], got["hit"] = np.ascontiguousarray(keys), np.asarray(hit, dtype=np.uint8)
    return got, assert_equals_restatement(got, N, G, (R, N, G, order), order, bw_scale)


# (E, N, C, G, sharpness, seed): N = 1027 is one LDS tile of records and a tail, G = 1000 no multiple of the workgroup, G = 4096 four tiles of
# the integration, N = 1 a degenerate row
SHAPES = [(1, 1, 2, 16, 1.0, 0), (3, 63, 10, 1000, 2.0, 1), (1, 300, 2, 1024, 1.0, 2), (3, 1027, 10, 4096, 2.0, 3), (3, 300, 10, 16, 2.0, 4),
          (1, 1027, 2, 1000, 1.0, 5), (3, 63, 2, 4096, 1.0, 6)]


def probs_of(E, N, C_, sharp, seed):
    ps, y = [], None
    for e in range(E):
        p, y0 = make_probs(N, C_, sharp * (1 + 0.5 * e), seed)               # (the same labels: the seed draws them second, from the same stream)
        y = y0 if y is None else y
        assert np.array_equal(y, y0)
        ps.append(p)
    return np.stack(ps), y


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "E{}N{}C{}G{}".format(*s[:4]))
def test_kernels_equal_the_numpy_restatement(shape):
    """Records written by bmi_reliability_record in uneven cuts into canary-padded buffers with spare columns, then the three kernels:
    every output bit for bit, twice, and once more from records written in one call"""
    E, N, C_, G, sharp, seed = shape
    p, y = probs_of(E, N, C_, sharp, seed)
    buf = Buffers(2 * E, N, G)
    record(buf, p, y, cuts_of(N))
    assert kde(buf) == _lib.BMI_OK
    got, intact = buf.read()
    assert intact
    host = reliability_numpy(p, y)
    assert np.array_equal(got["keys"], host["keys"]) and np.array_equal(got["hit"], host["hit"])
    want = assert_equals_restatement(got, N, G, shape)
    assert (want["n_data"] == N).all()
    if N == 1:
        assert (got["degenerate"] == 1).all() and (got["ece_kde"] == 0).all() and (got["density"] == 0).all()
    elif N >= 300:
        assert (got["degenerate"] == 0).all() and (got["ece_kde"] > 0).all()
    assert kde(buf) == _lib.BMI_OK
    assert same_bits(buf.read()[0], got)
    other = Buffers(2 * E, N, G)
    record(other, p, y, [N])
    assert kde(other) == _lib.BMI_OK
    again, intact = other.read()
    assert intact and same_bits(again, got, OUTPUTS + ("keys", "hit"))


def test_special_cases_of_the_host_file():
    """Tied two-class probabilities (mirror 2 - d), saturated images, the two clusters whose gap is carried across, order 2, a large and a
    small bandwidth factor"""
    p, y = make_probs(200, 2, 1.0, 5, lift=0.3)
    p[:40] = 0.5
    t = reliability_numpy(p[None], y)
    got, want = run_records(t["keys"], t["hit"], 1024)
    assert (t["keys"][:, :40] == np.float32(0.5).view(np.uint32)).all() and want["mirror_high"].all() and (got["degenerate"] == 0).all()
    p, y = make_probs(300, 10, 1.0, 6, lift=1.5)
    p[:30] = 0.0
    p[np.arange(30), y[:30]] = 1.0
    t = reliability_numpy(p[None], y)
    got, want = run_records(t["keys"], t["hit"], 1024)
    assert (t["keys"][:, :30] == 0x3f800000).all() and not want["mirror_high"].all() and (got["degenerate"] == 0).all()
    keys, hit = records_from(*two_clusters())
    for order in (1, 2):
        got, want = run_records(keys, hit, 2048, order)
        gap = (want["x"] > 0.5) & (want["x"] < 0.8)
        assert want["h"][0] < 0.1 and not want["is_set"][0][gap].any() and (want["integrand"][0][gap] > 0).all() and got["ece_kde"][0] > 0
    for scale in (2.0 ** -100, 1e-3, 50.0, 2.0 ** 100):                         # no grid point in reach ... every grid point under every centre
        got, want = run_records(keys, hit, 1000, 1, scale)
        assert all(np.isfinite(got[k]).all() for k in OUTPUTS) and got["degenerate"][0] == (scale < 1e-3)


def test_degenerate_rows_and_zero_keys():
    """The four degenerate kinds and a sound row in ONE call (rows are independent); records with key 0 are ignored"""
    N = 8
    keys, hit = np.zeros((5, N), dtype=np.uint32), np.zeros((5, N), dtype=np.uint8)
    for r, (conf, hb) in enumerate(DEGENERATE.values()):
        keys[r, 1:1 + len(conf)], hit[r, 1:1 + len(conf)] = np.asarray(conf, dtype=np.float32).view(np.uint32), hb
    keys[4], hit[4] = np.asarray([0.3, 0.9, 0.0, 0.8, 0.6, 0.0, 0.7, 0.95], dtype=np.float32).view(np.uint32), [0, 1, 1, 1, 0, 1, 1, 1]
    got, want = run_records(keys, hit, 1024, bw_scale=0.3)
    assert got["degenerate"].tolist() == [1, 1, 1, 1, 0] and (got["ece_kde"][:4] == 0).all() and got["ece_kde"][4] > 0
    assert got["n_data"].tolist() == [4, 4, 5, 0, 6] and got["n_hit"].tolist() == [0, 1, 3, 0, 4]
    assert all(np.isfinite(got[k]).all() for k in OUTPUTS) and (got["density"][:4] == 0).all()
    # the sound row's data alone, in order, give its bits
    data = keys[4] != 0
    alone, _ = run_records(keys[4:, data], hit[4:, data], 1024, bw_scale=0.3)
    assert same_bits({k: got[k][4:] for k in OUTPUTS}, alone)


def test_invalid_images_do_not_contribute():
    """A label out of range silences the image in every row, a non-finite probability the (row, image): key 0 — the rows equal those of
    the remaining images"""
    E, N, C_, G = 3, 63, 10, 1000
    p, y = probs_of(E, N, C_, 2.0, 8)
    bad, yb = p.copy(), y.copy()
    bad[1, 2, 3] = np.nan
    bad[0, 4, :] = np.inf
    yb[7], yb[8] = -1, C_
    buf = Buffers(2 * E, N, G)
    record(buf, bad, yb, cuts_of(N))
    assert kde(buf) == _lib.BMI_OK
    got, intact = buf.read()
    host = reliability_numpy(bad, yb)
    assert intact and np.array_equal(got["keys"], host["keys"]) and np.array_equal(got["hit"], host["hit"])
    assert_equals_restatement(got, N, G, "invalid images")
    assert got["n_data"].tolist() == [N - 3, N - 3, N - 2, N - 3, N - 4, N - 4] and all(np.isfinite(got[k]).all() for k in OUTPUTS)
    keep = np.ones(N, dtype=bool)
    keep[[7, 8]] = False
    rest = reliability_numpy(p[:, keep], y[keep])
    clean, _ = run_records(rest["keys"][2:3], rest["hit"][2:3], G, bw_scale=kde_bw_scale(N))
    assert same_bits({k: got[k][2:3] for k in OUTPUTS}, clean)                   # exit 2 has no non-finite value: its row is that of the 61 images


def test_an_error_writes_nothing():
    keys, hit = records_from(*two_clusters(300))
    buf = Buffers(1, 300, 1024)
    buf.put(keys, hit)
    INVALID, UNSUPPORTED = -22, -95
    for name in ("keys", "hit") + OUTPUTS:
        assert kde(buf, **{name: None}) == INVALID, name
    for change in (dict(R=0), dict(N=0), dict(N=buf.cap + 1), dict(G=15), dict(G=65537), dict(order=0), dict(order=3), dict(bw_scale=0.0),
                   dict(bw_scale=-1.0), dict(bw_scale=float("nan")), dict(bw_scale=float("inf"))):
        assert kde(buf, **change) == INVALID, change
    for change in (dict(R=65), dict(bw_scale=2.0 ** -101), dict(bw_scale=2.0 ** 101)):
        assert kde(buf, **change) == UNSUPPORTED, change
    assert buf.read()[1] and buf.all_as_filled(OUTPUTS)
    assert kde(buf) == _lib.BMI_OK and not buf.all_as_filled(OUTPUTS)


KW = dict(dropout_exit=True, dropout="block", dropout_p=0.25, out_dim=10)


def _model():
    m = synthetic_weights_(build_seeded(ResNet18MCEarlyExit, KW), 0).to(DEV).eval()
    m.engine_dtype = "f16x2"
    return m


def test_engine_method_and_graph_capture():
    """MCDEngine.reliability_kde against the restatement, its argument and degenerate-row errors, and ONE torch.cuda.graph capture of record
    + kde whose replays give the eager bits, also on new inputs"""
    eng = MCDEngine(_model(), DEV, max_batch=8, dtype="f16x2")
    E, N, C_, G = 4, 300, 10, 1024
    p, y = probs_of(E, N, C_, 2.0, 9)
    rec = eng.new_reliability_records(N + 5)
    pd, yd = torch.from_numpy(p).to(DEV), torch.from_numpy(y)
    assert eng.reliability_records(pd[:, :100].contiguous(), yd[:100], rec, 0) == 100
    assert eng.reliability_records(pd[:, 100:].contiguous(), yd[100:], rec, 100) == N
    host = reliability_numpy(p, y)

    def check(out, host, order=1, G=G):
        got = {k: out[k].cpu().numpy() for k in OUTPUTS}
        got["keys"], got["hit"] = host["keys"], host["hit"]
        assert tuple(out["density"].shape) == (2 * E, 2, G) and out["n_data"].dtype == torch.int64 and out["degenerate"].dtype == torch.int32
        return assert_equals_restatement(got, N, G, ("engine", order, G), order)

    eager = eng.reliability_kde(rec, N, G)
    check(eager, host)
    check(eng.reliability_kde(rec, N, 1000, order=2), host, 2, 1000)
    w = reliability_kde_numpy(host["keys"], host["hit"], N, G, bw_scale=0.25)
    assert np.array_equal(eng.reliability_kde(rec, N, G, bw_scale=0.25)["ece_kde"].cpu().numpy(), w["ece_kde"])
    for bad in (dict(n=N + 6), dict(n=0), dict(grid_points=15), dict(grid_points=2 ** 16 + 1), dict(order=3), dict(bw_scale=0.0),
                dict(bw_scale=float("nan"))):
        with pytest.raises(ValueError):
            eng.reliability_kde(rec, **{"n": N, "grid_points": G, **bad})
    # graph capture: static inputs, the outputs allocated inside the capture
    ps, ys = pd.clone(), yd.to(DEV).clone()
    out = {}
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        eng.reliability_records(ps, ys, rec, 0)
        out.update(eng.reliability_kde(rec, N, G, check=False))
    graph.replay()
    torch.cuda.synchronize()
    assert all(torch.equal(out[k], eager[k]) for k in OUTPUTS)
    p2, y2 = probs_of(E, N, C_, 3.0, 10)
    ps.copy_(torch.from_numpy(p2))
    ys.copy_(torch.from_numpy(y2))
    graph.replay()
    torch.cuda.synchronize()
    check(out, reliability_numpy(p2, y2))
    # a degenerate row: the last exit always right with confidence 1.0 — its hit confidences are all equal —, its ensemble row is not
    p3 = p.copy()
    p3[3] = 0.0
    p3[3, np.arange(N), y] = 1.0
    eng.reliability_records(torch.from_numpy(p3).to(DEV), yd, rec, 0)
    with pytest.raises(ValueError, match=r"rows.*: 3$"):
        eng.reliability_kde(rec, N, G)
    quiet = eng.reliability_kde(rec, N, G, check=False)
    assert quiet["degenerate"].tolist() == [0, 0, 0, 1, 0, 0, 0, 0] and quiet["ece_kde"][3] == 0 and row_names(E)[3] == "3"
    assert not any(torch.isnan(v).any() for v in quiet.values())


def test_reliability_analysis_kde_against_full_analysis(tmp_path, monkeypatch):
    """The seeded ResNet-18, N = 96 in 3 uneven batches, T = 4: ``kde`` equals the restatement on the walk's own records bit for bit and
    ece_kde_binary(method="direct") on the preds FullAnalysis collects for the same seed within 1e-7 (a degenerate row: NaN on both sides);
    kde=False gives the rows and the CSV of the walk without it."""
    m = synthetic_weights_(build_seeded(ResNet18MCEarlyExit, KW), 0).to(DEV).eval()
    N, T, seed, G = 96, 4, 11, 1024
    x, y = synthetic_images(N, seed=3), synthetic_labels(N, 10, seed=4)
    loader = [(x[a:b], y[a:b]) for a, b in ((0, 40), (40, 72), (72, 96))]
    fa = FullAnalysis(m, loader, gpu=0, mc_dropout=True, mc_passes=T, seed=seed, macro_batches=1, ece="hist")
    plain = ReliabilityAnalysis(m, loader, gpu=0, mc_passes=T, seed=seed)
    ra = ReliabilityAnalysis(m, loader, gpu=0, mc_passes=T, seed=seed, kde=True, grid_points=G)
    E = fa.preds.shape[0]
    assert plain.kde is False and "ece_kde" not in plain.metrics and all(len(r) == 6 for r in plain.rows)
    assert [r[:6] for r in ra.rows] == plain.rows and ra.n == N
    got = {k: ra.kde[k].cpu().numpy() for k in OUTPUTS}
    got["keys"] = np.ascontiguousarray(ra.records["keys"][:, :N].cpu().numpy()).view(np.uint32)
    got["hit"] = ra.records["hit"][:, :N].cpu().numpy()
    assert np.array_equal(got["keys"], reliability_numpy(fa.preds, fa.labels.argmax(1))["keys"])
    assert_equals_restatement(got, N, G, "walk")
    deg = got["degenerate"] != 0
    print(f"walk: degenerate rows {np.nonzero(deg)[0].tolist()}, n_hit {got['n_hit'].tolist()}")
    assert np.array_equal(np.isnan(ra.metrics["ece_kde"]), deg) and np.array_equal(ra.metrics["ece_kde"][~deg], got["ece_kde"][~deg])
    worst = 0.0
    for r, row in enumerate(ra.rows):
        v = (fa.preds if r < E else fa.ensemble_preds)[r % E]
        with np.errstate(invalid="ignore", divide="ignore"):
            direct = ece_kde_binary(v, fa.labels, grid_points=G, method="direct")
        assert len(row) == 7 and (np.isnan(row[6]) and np.isnan(direct) if deg[r] else row[6] == got["ece_kde"][r])
        if not deg[r]:
            worst = max(worst, abs(row[6] - direct))
    print(f"walk: max |ece_kde - ece_kde_binary(direct)| = {worst:.2e}")
    assert worst <= DIRECT_BOUND and not deg.all()
    monkeypatch.chdir(tmp_path)
    lines = open(ra.save("k")).read().splitlines()
    assert lines[0] == "Layer,Accuracy,ECE,MCE,NLL,Brier,ECE_KDE" and len(lines) == 1 + 2 * E and len(lines[1].split(",")) == 7
    assert [float(l.split(",")[6]) for l in np.array(lines[1:])[~deg]] == [r[6] for r, d in zip(ra.rows, deg) if not d]
    today = open(plain.save("p")).read().splitlines()
    assert today[0] == "Layer,Accuracy,ECE,MCE,NLL,Brier" and today[1:] == [",".join(str(v) for v in r) for r in plain.rows]
    assert [l.rsplit(",", 1)[0] for l in lines[1:]] == today[1:]
