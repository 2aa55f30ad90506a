"""-m gpu: per-pass multi-exit accuracy on the device (bmi_pass_accuracy, MCDEngine.pass_accuracy) — the kernel against its numpy
restatement (counts equal exactly, the max-probability sums to 1e-12), reproducibility, the tie rule, non-finite rows and bad labels,
errors that write nothing — and the two callers: evaluate(device_metrics=True) against the reference's own evaluate() and against the
torch route, evaluate_exits against the restatement applied to the same walk's per-sample logits."""
import ctypes as C

import numpy as np
import pytest
import torch

from bayesnn_fpga_amd import _lib
from bayesnn_fpga_amd.engine import MCDEngine
from bayesnn_fpga_amd.models.resnet18.resnet18 import ResNet18MCEarlyExit
from bayesnn_fpga_amd.synthetic import synthetic_images, synthetic_labels, synthetic_weights_
from bayesnn_fpga_amd.train.evaluate import (MultiExitAccuracy, _fraction, evaluate, evaluate_exits, exit_metric_names,
                                             pass_accuracy_numpy)
from tests.gpu_helpers import ptr, stream
from tests.helpers import build_seeded, golden_kwargs, load_golden
from tests.test_pass_accuracy_host import CASES, TOPS, _tied_case, make_case, tie_gap

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
PAD = 16                      # canary entries in front of and behind each output


def run_kernel(l, y, tops, scratch_bytes=None, count=True):
    """bmi_pass_accuracy through the C ABI on NaN / -1 filled outputs with canaries around them -> (rc, hits, maxprob, nonfinite, intact)"""
    lib = _lib.lib()
    T, E, B, C_ = l.shape
    K = len(tops)
    ld, yd = torch.from_numpy(l).to(DEV), torch.from_numpy(np.asarray(y).astype(np.int32)).to(DEV)
    hits = torch.full((PAD + T * 2 * E * K + PAD,), -7, dtype=torch.int32, device=DEV)
    maxprob = torch.full((PAD + T * E + PAD,), float("nan"), dtype=torch.float64, device=DEV)
    nf = torch.full((1,), 100, dtype=torch.int32, device=DEV)
    need = int(lib.bmi_pass_accuracy_scratch_bytes(T, E, B))
    assert need == T * E * B * 16
    scratch = torch.empty(need if scratch_bytes is None else max(scratch_bytes, 1), dtype=torch.uint8, device=DEV)
    rc = lib.bmi_pass_accuracy(ptr(ld), T, E, B, C_, ptr(yd), (C.c_int32 * K)(*tops), K, C.c_void_p(hits.data_ptr() + 4 * PAD),
                               C.c_void_p(maxprob.data_ptr() + 8 * PAD), ptr(nf) if count else None, ptr(scratch),
                               need if scratch_bytes is None else scratch_bytes, stream())
    torch.cuda.synchronize()
    h, m = hits.cpu().numpy(), maxprob.cpu().numpy()
    intact = (h[:PAD] == -7).all() and (h[-PAD:] == -7).all() and np.isnan(m[:PAD]).all() and np.isnan(m[-PAD:]).all()
    return rc, h[PAD:-PAD].reshape(T, 2, E, K), m[PAD:-PAD].reshape(T, E), int(nf.item()) - 100, bool(intact)


KERNEL_CASES = CASES[:5] + [(2, 32, 3, 65, 3, 6), (1, 4, 1, 10, 3, 7)]


@pytest.mark.parametrize("case", KERNEL_CASES, ids=lambda c: "T{}E{}B{}C{}".format(*c[:4]))
def test_kernel_equals_its_numpy_restatement(case):
    """hits equal exactly on tie-free input (the least relative gap of an ensemble score to the label's is >= 1e-6, five orders above what
    the device's exp and its summation tree can move), maxprob to 1e-12 relative (tests/test_temperature.py: the tolerance the project's
    float64 kernels hold against their restatements); two runs give the same bits; canaries untouched."""
    l, y = make_case(*case)
    no_equal, gap = tie_gap(l, y)
    assert no_equal and gap >= 1e-6
    want_h, want_m, _ = pass_accuracy_numpy(l, y, TOPS)
    rc, h, m, nf, intact = run_kernel(l, y, TOPS)
    assert rc == _lib.BMI_OK and intact and nf == 0
    print(f"{case}: hit-count differences {int((h != want_h).sum())}, max relative maxprob difference {float(np.abs(m / want_m - 1).max()):.2e}")
    assert np.array_equal(h, want_h)
    np.testing.assert_allclose(m, want_m, rtol=1e-12, atol=0)
    rc2, h2, m2, _, _ = run_kernel(l, y, TOPS)
    assert rc2 == _lib.BMI_OK and np.array_equal(h, h2) and np.array_equal(m.view(np.int64), m2.view(np.int64))
    # eight cut-offs, one beyond C; without a counter
    tops8 = (1, 2, 3, 5, 7, 11, case[3], case[3] + 5)
    rc, h8, m8, nf, intact = run_kernel(l, y, tops8, count=False)
    assert rc == _lib.BMI_OK and intact and nf == 0
    assert np.array_equal(h8, pass_accuracy_numpy(l, y, tops8)[0]) and (h8[..., -1] == case[2]).all()
    assert np.array_equal(m8.view(np.int64), m.view(np.int64))


def test_the_tie_rule_non_finite_rows_and_bad_labels():
    l, y = _tied_case()
    tops = (1, 2, 5, 9, 12)
    rc, h, m, nf, intact = run_kernel(l, y, tops)
    want_h, want_m, _ = pass_accuracy_numpy(l, y, tops)
    assert rc == _lib.BMI_OK and intact and nf == 0 and np.array_equal(h, want_h)
    np.testing.assert_allclose(m, want_m, rtol=1e-12, atol=0)
    # a NaN row, +inf rows, a -inf entry, labels -1 and C: misses, counted, the other rows as they were
    l, y = make_case(3, 4, 11, 10, 3, 9)
    rc, h0, m0, nf, _ = run_kernel(l, y, (1, 5, 11))
    assert rc == _lib.BMI_OK and nf == 0
    bad, yb = l.copy(), y.copy()
    bad[0, 1, 2, 3] = np.nan
    bad[1, 0, 4, :] = np.inf
    bad[2, 3, 5, 0] = -np.inf
    yb[7], yb[8] = -1, 10
    rc, h, m, nf, intact = run_kernel(bad, yb, (1, 5, 11))
    want_h, want_m, want_nf = pass_accuracy_numpy(bad, yb, (1, 5, 11))
    assert rc == _lib.BMI_OK and intact and nf == want_nf == 3
    assert np.isfinite(m).all() and np.array_equal(h, want_h)
    np.testing.assert_allclose(m, want_m, rtol=1e-12, atol=0)
    assert (h <= h0).all() and (h < h0).any()
    untouched = np.ones((3, 4), dtype=bool)
    untouched[0, 1] = untouched[1, 0] = untouched[2, 3] = False
    assert np.array_equal(m.view(np.int64)[untouched], m0.view(np.int64)[untouched])       # the other rows' sums keep their bits
    # the same images alone: every count of the clean images is what the clean run gave them
    clean = [b for b in range(11) if b not in (2, 4, 5, 7, 8)]
    rc, hc, _, _, _ = run_kernel(np.ascontiguousarray(bad[:, :, clean]), yb[clean], (1, 5, 11))
    rc2, hc0, _, _, _ = run_kernel(np.ascontiguousarray(l[:, :, clean]), y[clean], (1, 5, 11))
    assert rc == rc2 == _lib.BMI_OK and np.array_equal(hc, hc0)


def test_an_error_writes_nothing():
    l, y = make_case(2, 3, 9, 10, 3, 11)
    for kwargs in (dict(scratch_bytes=2 * 3 * 9 * 16 - 1), ):
        rc, h, m, nf, intact = run_kernel(l, y, TOPS, **kwargs)
        assert rc == -12 and intact and nf == 0 and (h == -7).all() and np.isnan(m).all()
    rc, h, m, nf, intact = run_kernel(l, y, (1, 0))
    assert rc == -22 and intact and nf == 0 and (h == -7).all() and np.isnan(m).all()
    rc, h, m, nf, intact = run_kernel(l, y, tuple(range(1, 10)))
    assert rc == -95 and intact and nf == 0 and (h == -7).all() and np.isnan(m).all()


def test_fraction_is_torch_s_fp32_mean_on_the_gpu():
    """Every count of 0 / 1 values over B images, B not a power of two: torch's mean on the device (over an inner axis, as _metrics_passes
    takes it, and over a whole vector) is float32(count) * float32(1 / B), the form the device route assembles its accuracies with."""
    for B in (7, 12, 37, 250):
        v = (torch.arange(B, device=DEV)[None, :, None] < torch.arange(B + 1, device=DEV)[:, None, None]).float().expand(B + 1, B, 2).contiguous()
        want = _fraction(np.arange(B + 1), B)
        assert np.array_equal(v.mean(dim=1)[:, 0].double().cpu().numpy(), want), B
        assert np.array_equal(np.array([float(v[c, :, 0].contiguous().mean()) for c in range(0, B + 1, 3)]), want[::3]), B
    assert (_fraction(np.arange(13), 12) != _fraction(np.arange(13), 12, gpu_mean=False)).any()


def _model(kw, dtype="f16x2"):
    m = synthetic_weights_(build_seeded(ResNet18MCEarlyExit, kw), 0).to(DEV).eval()
    m.engine_dtype = dtype
    return m


def test_engine_pass_accuracy_out_and_nonfinite():
    """MCDEngine.pass_accuracy: fresh outputs, the caller's buffers (a row of a table), the counter; a NaN fed through out= / nonfinite="""
    m = _model(dict(dropout_exit=True, dropout="block", dropout_p=0.25, out_dim=10))
    eng = MCDEngine(m, DEV, max_batch=8, dtype="f16x2")
    l, y = make_case(3, 4, 8, 10, 3, 12)
    ld = torch.from_numpy(l).to(DEV)
    hits, maxprob = eng.pass_accuracy(ld, torch.from_numpy(y))
    want_h, want_m, _ = pass_accuracy_numpy(l, y, TOPS)
    assert hits.dtype == torch.int32 and tuple(hits.shape) == (3, 2, 4, 2) and maxprob.dtype == torch.float64
    assert np.array_equal(hits.cpu().numpy(), want_h)
    np.testing.assert_allclose(maxprob.cpu().numpy(), want_m, rtol=1e-12, atol=0)
    table_h = torch.full((2, 3, 2, 4, 2), -1, dtype=torch.int32, device=DEV)
    table_m = torch.full((2, 3, 4), float("nan"), dtype=torch.float64, device=DEV)
    nf = torch.zeros(1, dtype=torch.int32, device=DEV)
    ld[1, 2, 3, 4] = float("nan")
    out = eng.pass_accuracy(ld, torch.from_numpy(y), TOPS, out=(table_h[1], table_m[1]), nonfinite=nf)
    assert out[0].data_ptr() == table_h[1].data_ptr() and int(nf.item()) == 1
    bad = l.copy()
    bad[1, 2, 3, 4] = np.nan
    want_h, want_m, _ = pass_accuracy_numpy(bad, y, TOPS)
    assert np.array_equal(table_h[1].cpu().numpy(), want_h) and (table_h[0] == -1).all() and torch.isnan(table_m[0]).all()
    np.testing.assert_allclose(table_m[1].cpu().numpy(), want_m, rtol=1e-12, atol=0)
    eng.pass_accuracy(ld, torch.from_numpy(y), TOPS, out=(table_h[0], table_m[0]), nonfinite=nf)
    assert int(nf.item()) == 2                                                   # ADDED to
    with pytest.raises(ValueError):
        eng.pass_accuracy(ld, torch.from_numpy(y), TOPS, out=(table_h[0].float(), table_m[0]))
    with pytest.raises(ValueError):
        eng.pass_accuracy(ld, torch.from_numpy(y), (1, 2, 3), out=(table_h[0], table_m[0]))
    with pytest.raises(ValueError):
        eng.pass_accuracy(ld, torch.from_numpy(y[:5]))
    with pytest.raises(_lib.BmiError):
        eng.pass_accuracy(ld, torch.from_numpy(y), (1, 0))


def test_evaluate_device_metrics_against_the_reference_s_own_evaluate_and_the_torch_route():
    """tests/golden/evaluate_masksembles.npz under the conditions of tests/test_collation.py's folded-evaluate test, on f16x2: accuracies
    to 1e-6, avg_maxprob to 1e-5, counters where the reference's end; against the torch route on the same model the accuracy entries are
    equal exactly, avg_maxprob within 1e-6 (torch's fp32 softmax and mean against float64)."""
    g = load_golden("evaluate_masksembles.npz")
    kw = golden_kwargs(g)
    B, nb, T, cnt0 = int(g["B"]), int(g["nb"]), int(g["T"]), int(g["cnt0"])
    x, y = synthetic_images(B * nb, seed=3), synthetic_labels(B * nb, 10, seed=4)
    loader = [(x[i * B:(i + 1) * B], y[i * B:(i + 1) * B]) for i in range(nb)]
    loss = MultiExitAccuracy(4, acc_tops=(1, 5))
    want = g["averaged"]
    got = {}
    for device_metrics in (True, False):
        m = _model(kw)
        for lay in m.mask_layers():
            lay.cnt = cnt0
        got[device_metrics] = np.array(evaluate(loss, loader, m, 0, "t", T, create_log=False, device_metrics=device_metrics))
        assert {lay.cnt for lay in m.mask_layers()} == {int(g["cnt_after"])} and m.mc_pass == T * nb
    dev, tor = got[True], got[False]
    print(f"device route: max|acc - ref| = {np.abs(dev[:-1] - want[:-1]).max():.2e}, |maxprob - ref| = {abs(dev[-1] - want[-1]):.2e}, "
          f"|maxprob - torch route| = {abs(dev[-1] - tor[-1]):.2e}")
    np.testing.assert_allclose(dev[:-1], want[:-1], rtol=0, atol=1e-6)
    assert abs(dev[-1] - want[-1]) <= 1e-5
    assert np.array_equal(dev[:-1], tor[:-1])
    assert abs(dev[-1] - tor[-1]) <= 1e-6


@pytest.mark.parametrize("kind", ["mc", "mask"])
def test_evaluate_exits_equals_the_restatement_on_the_walk_s_own_logits(kind):
    """A 3-batch loader with a smaller last batch, B = 12, T = 5: the dict equals pass_accuracy_numpy applied to forward_samples of the same
    walk (same seeds, sample indices and Masksembles counters), averaged over the batches per pass, then over the passes; the last exit's
    row is evaluate()'s acc{i}_clf0 from the same state; acc_ens[0] == acc_clf[0]; the std entries are np.std of the per-pass tables."""
    kw = dict(dropout_exit=True, dropout="block", dropout_p=0.25, out_dim=10)
    if kind == "mask":
        kw.update(mask_type="mask", num_masks=4, mask_scale=4.0)
    B, T, sizes = 12, 5, (12, 12, 7)
    x, y = synthetic_images(sum(sizes), seed=21), synthetic_labels(sum(sizes), 10, seed=22)
    off = np.concatenate([[0], np.cumsum(sizes)])
    loader = [(x[off[i]:off[i + 1]], y[off[i]:off[i + 1]]) for i in range(3)]
    nb, E, K = 3, 4, 2
    m = _model(kw)
    m.mc_pass = 3
    for lay in m.mask_layers():
        lay.cnt = 2
    cnt = m.mask_layers()[0].cnt if m.mask_layers() else 0
    eng = MCDEngine(m, DEV, max_batch=B, dtype="f16x2")
    rows = np.zeros((nb, T, 2 * E * K + E))
    for k, (X, yy) in enumerate(loader):
        lg = eng.forward_samples(X.to(DEV), T, seed=m.mc_seed, t_begin=m.mc_pass + k * T, cnt0=cnt + k, mask_stride=nb).cpu().numpy()
        h, mp, nf = pass_accuracy_numpy(lg, yy.numpy(), TOPS)
        assert nf == 0
        inv = np.float32(1) / np.float32(len(yy))                                # (torch's fp32 mean on the GPU: the sum times float32(1 / B))
        rows[k] = np.concatenate([(h.astype(np.float32) * inv).astype(np.float64).reshape(T, -1), mp / len(yy)], axis=1)
    per_pass = np.array([[sum(float(rows[k, i, j]) for k in range(nb)) / nb for j in range(rows.shape[2])] for i in range(T)])
    r = evaluate_exits(loader, m, 0, T, acc_tops=TOPS)
    assert m.mc_pass == 3 + T * nb and {lay.cnt for lay in m.mask_layers()} <= {(2 + T * nb) % 4}
    assert r["names"] == exit_metric_names(E, TOPS) and r["acc_tops"] == TOPS
    assert r["acc_clf_passes"].shape == (T, E, K) and r["acc_ens_passes"].shape == (T, E, K) and r["maxprob_passes"].shape == (T, E)
    assert np.array_equal(r["acc_clf_passes"], per_pass[:, :E * K].reshape(T, E, K))
    assert np.array_equal(r["acc_ens_passes"], per_pass[:, E * K:2 * E * K].reshape(T, E, K))
    np.testing.assert_allclose(r["maxprob_passes"], per_pass[:, 2 * E * K:], rtol=1e-12, atol=0)
    for name in ("acc_clf", "acc_ens", "maxprob"):
        assert np.array_equal(r[name], np.average(r[name + "_passes"], axis=0))
        assert np.array_equal(r[name + "_std"], np.std(r[name + "_passes"], axis=0))
    assert np.array_equal(r["acc_ens"][0], r["acc_clf"][0]) and np.array_equal(r["acc_ens_passes"][:, 0], r["acc_clf_passes"][:, 0])
    assert 0.0 < r["acc_clf"][:, 1].min() and r["acc_clf"][:, 0].max() < 1.0 and (r["maxprob"] > 0.1).all()
    # evaluate() from the same state: its vector holds the last exit (as clf0, the reference's row-0 overwrite) and avg_maxprob; the full
    # ensemble lands in a row the reference never emits, so the vector has no entry to compare acc_ens[E - 1] with
    loss = MultiExitAccuracy(4, acc_tops=TOPS)
    for device_metrics in (False, True):
        m.mc_pass = 3
        for lay in m.mask_layers():
            lay.cnt = 2
        vec = dict(zip(loss.metric_names, evaluate(loss, loader, m, 0, "t", T, create_log=False, device_metrics=device_metrics)))
        for i, top in enumerate(TOPS):
            assert vec[f"acc{top}_clf0"] == r["acc_clf"][E - 1, i], (device_metrics, top)
            assert vec[f"acc{top}_avg"] == r["acc_clf"][E - 1, i] / 4
        assert abs(vec["avg_maxprob"] - r["maxprob"][E - 1]) <= 1e-6


def test_evaluate_raises_on_the_kernel_s_non_finite_counter(monkeypatch):
    """A NaN written into one logit of one batch behind the engine pass: the device route raises the torch route's FloatingPointError from
    the counter after the walk's synchronisation, and the model's pass index has not moved."""
    kw = dict(dropout_exit=True, dropout="block", dropout_p=0.25, out_dim=10)
    m = _model(kw)
    x, y = synthetic_images(8, seed=5), synthetic_labels(8, 10, seed=6)
    loader = [(x[:4], y[:4]), (x[4:], y[4:])]
    loss = MultiExitAccuracy(4, acc_tops=TOPS)
    real = MCDEngine.forward_samples
    calls = []

    def poisoned(self, *a, **k):
        out = real(self, *a, **k)
        calls.append(1)
        if len(calls) == 2:
            out[1, 2, 3, 4] = float("nan")
        return out
    monkeypatch.setattr(MCDEngine, "forward_samples", poisoned)
    monkeypatch.setattr(torch, "isfinite", lambda *a, **k: pytest.fail("the device route read the logits through torch.isfinite"))
    with pytest.raises(FloatingPointError, match="non-finite logits on the 'f16x2' engine"):
        evaluate(loss, loader, m, 0, "t", 3, create_log=False, device_metrics=True)
    assert len(calls) == 2 and m.mc_pass == 0
