"""-m gpu: vote counts on the device (csrc/votes.hip: bmi_vote_counts / bmi_forward_mcd_votes / bmi_finalize_votes) — the kernel against
its numpy restatement for every case x calibration map x plain / weighted ensembles (counts equal exactly on gap-checked input),
additivity, ties, non-finite rows, errors that write nothing, the read-out, the engine path against the stand-alone entry on the engine's
own per-sample logits, graph capture, and UncertaintyAnalysis(votes=True)."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from bayesnn_fpga_amd import _lib
from bayesnn_fpga_amd.engine import MCDEngine
from bayesnn_fpga_amd.models.resnet18.resnet18 import ResNet18MCEarlyExit
from bayesnn_fpga_amd.synthetic import synthetic_images, synthetic_labels, synthetic_weights_
from bayesnn_fpga_amd.train.uncertainty import UncertaintyAnalysis, vote_counts_numpy, vote_readout_numpy
from tests.gpu_helpers import ptr, stream
from tests.helpers import build_seeded
from tests.test_pass_accuracy_host import make_case
from tests.test_votes_host import CASES, GAP, MAPS, bad_case, case_id, make_map, make_weights, vote_gap

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
PAD = 16                      # canary entries in front of and behind the counts
FILL = 5                      # what the counts hold before a call: they are ADDED to


def _dev(a):
    return None if a is None else torch.from_numpy(np.array(a)).to(DEV)      # (a copy: the shared references are read-only)


def run_kernel(l, weights=None, tau=None, scale=None, bias=None, matrix=None, into=None, count=True, shape=None):
    """bmi_vote_counts through the C ABI on counts pre-filled with FILL (or ``into``, a device tensor of an earlier call) with canaries
    around them -> (rc, V - FILL, the counter's gain, canaries intact, the device tensor)"""
    lib = _lib.lib()
    T, E, B, C_ = shape or l.shape
    n = 2 * E * B * C_
    ld = _dev(l)
    if into is None:
        into = torch.full((PAD + n + PAD,), -7, dtype=torch.int32, device=DEV)
        into[PAD:PAD + n] = FILL
    nf = torch.full((1,), 100, dtype=torch.int32, device=DEV)
    tau_c = None if tau is None else (C.c_float * E)(*np.asarray(tau, dtype=np.float64).tolist())
    keep = [_dev(scale), _dev(bias), _dev(matrix), _dev(weights)]
    rc = lib.bmi_vote_counts(ptr(ld), T, E, B, C_, tau_c, ptr(keep[0]), ptr(keep[1]), ptr(keep[2]), ptr(keep[3]),
                             C.c_void_p(into.data_ptr() + 4 * PAD), ptr(nf) if count else None, stream())
    torch.cuda.synchronize()
    v = into.cpu().numpy()
    intact = bool((v[:PAD] == -7).all() and (v[-PAD:] == -7).all())
    return rc, v[PAD:-PAD].reshape(2, E, B, C_) - FILL, int(nf.item()) - 100, intact, into


@functools.lru_cache(maxsize=None)
def reference(case, kind, weighted):
    """(logits, the map's keyword arguments, W or None, the restatement's V) of one case: computed once, shared, never written to"""
    l, _ = make_case(*case)
    T, E, B, C_ = l.shape
    cal = make_map(kind, E, C_, case[5])
    W = make_weights(E, case[5]) if weighted else None
    no_equal, gap = vote_gap(l, weights=W, **cal)
    print(f"{case} {kind} weighted={weighted}: least relative top-2 gap of q {gap:.2e}")
    assert no_equal and gap >= GAP                 # (a condition on the input, not a measurement of the code)
    V, nf = vote_counts_numpy(l, weights=W, **cal)
    assert nf == 0
    for a in (l, V):
        a.setflags(write=False)
    return l, cal, W, V


@pytest.mark.parametrize("weighted", [False, True], ids=["mean", "weighted"])
@pytest.mark.parametrize("kind", MAPS)
@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_kernel_equals_its_numpy_restatement(case, kind, weighted):
    """V[0] equals always (both sides compare the same fp32 numbers), V[1] on input whose least relative top-2 gap of any q row is >= 1e-6
    (five orders above what the device's exp and its summation tree can move); pre-filled counts are added to; two runs give the same
    bits; canaries untouched."""
    l, cal, W, want = reference(case, kind, weighted)
    rc, V, nf, intact, _ = run_kernel(l, weights=W, **cal)
    assert rc == _lib.BMI_OK and intact and nf == 0
    print(f"{case} {kind} weighted={weighted}: differing counts V[0] {int((V[0] != want[0]).sum())}, V[1] {int((V[1] != want[1]).sum())}")
    assert np.array_equal(V[0], want[0])
    assert np.array_equal(V[1], want[1])
    rc2, V2, _, _, _ = run_kernel(l, weights=W, count=False, **cal)
    assert rc2 == _lib.BMI_OK and np.array_equal(V, V2)


@pytest.mark.parametrize("kind,weighted", [("none", False), ("tau", True), ("matrix", False)])
def test_additivity_over_the_split_of_t(kind, weighted):
    """Two calls on the halves of T into one V equal one call (and the counts that were there stay: FILL)"""
    case = CASES[6]                                # T = 5: halves of 2 and 3
    l, cal, W, want = reference(case, kind, weighted)
    rc, _, _, _, buf = run_kernel(np.ascontiguousarray(l[:2]), weights=W, **cal)
    rc2, V, nf, intact, _ = run_kernel(np.ascontiguousarray(l[2:]), weights=W, into=buf, **cal)
    assert rc == rc2 == _lib.BMI_OK and intact and nf == 0
    assert np.array_equal(V, want)
    assert (V.sum(-1) == case[0]).all()


def test_constructed_ties():
    l = np.zeros((1, 1, 3, 5), np.float32)
    l[0, 0, 0, [1, 3]] = 2.0
    l[0, 0, 1, [4, 0]] = 1.0
    l[0, 0, 2, :] = -3.0
    rc, V, nf, intact, _ = run_kernel(l)
    assert rc == _lib.BMI_OK and intact and nf == 0
    assert np.array_equal(V, vote_counts_numpy(l)[0]) and V[0, 0].argmax(-1).tolist() == [1, 0, 0] and np.array_equal(V[1], V[0])
    # ties across the lane halves: classes 3, 64 + 3 and 127 tied at the top -> 3; only 70 and 127 -> 70
    l = np.zeros((1, 1, 2, 128), np.float32)
    l[0, 0, 0, [3, 67, 127]] = 1.5
    l[0, 0, 1, [70, 127]] = 1.5
    rc, V, _, _, _ = run_kernel(l)
    assert rc == _lib.BMI_OK and np.array_equal(V, vote_counts_numpy(l)[0])
    assert V[:, 0, 0].argmax(-1).tolist() == [3, 3] and V[:, 0, 1].argmax(-1).tolist() == [70, 70]
    # equal q from mirrored exits (classes 0 and 1 swapped: the same pairs in the butterfly, a + b == b + a): the lower class
    l = np.zeros((2, 2, 1, 4), np.float32)
    l[:, 0, 0] = [3.0, 1.0, 0.0, -1.0]
    l[:, 1, 0] = [1.0, 3.0, 0.0, -1.0]
    rc, V, _, _, _ = run_kernel(l)
    assert rc == _lib.BMI_OK
    assert V[0, :, 0].tolist() == [[2, 0, 0, 0], [0, 2, 0, 0]] and V[1, :, 0].tolist() == [[2, 0, 0, 0], [2, 0, 0, 0]]


@pytest.mark.parametrize("scaled", [False, True], ids=["raw", "scaled"])
def test_non_finite_rows(scaled):
    """A NaN logit, a row of +inf, a -inf entry, an inf the scale makes of a finite logit: no vote from the row or from the ensembles behind
    it, the counter equals the restatement's, every other row's counts are what they were."""
    clean, l, cal, rows = bad_case(scaled)
    no_equal, gap = vote_gap(clean, **cal)
    assert no_equal and gap >= GAP                 # (the rows that still vote are the clean input's: a condition on the input)
    with np.errstate(over="ignore"):
        want, want_nf = vote_counts_numpy(l, **cal)
    rc, V, nf, intact, _ = run_kernel(l, **cal)
    assert rc == _lib.BMI_OK and intact and nf == want_nf == len(rows)
    assert np.array_equal(V, want)
    rc, Vc, nfc, _, _ = run_kernel(clean, **cal)
    assert rc == _lib.BMI_OK and nfc == 0
    untouched = [b for b in range(11) if b not in {r[2] for r in rows}]
    assert np.array_equal(V[:, :, untouched], Vc[:, :, untouched]) and (V <= Vc).all() and (V < Vc).any()
    # every row bad: nothing is counted, the read-out gives its sentinels
    rc, V, nf, intact, _ = run_kernel(np.full((2, 2, 3, 4), np.nan, np.float32))
    assert rc == _lib.BMI_OK and intact and nf == 12 and not V.any()


def test_an_error_writes_nothing():
    l, _ = make_case(2, 3, 9, 10, 3, 11)
    a = np.ones((3, 10), np.float32)
    for want, kw in ((-22, dict(tau=[1.0, 1.0, 1.0], scale=a, bias=a)), (-22, dict(tau=[1.0, 0.0, 1.0])), (-22, dict(bias=a)),
                     (-22, dict(scale=a)), (-22, dict(shape=(0, 3, 9, 10))), (-95, dict(shape=(1, 1, 1, 129))), (-95, dict(shape=(1, 33, 1, 1)))):
        rc, V, nf, intact, _ = run_kernel(l, **kw)
        assert rc == want and intact and nf == 0 and not V.any(), kw


def run_finalize(V):
    """bmi_finalize_votes through the C ABI on V [2, E, B, C] -> (rc, vote_class, variation_ratio, vote_entropy), each [2, E, B]"""
    lib = _lib.lib()
    _, E, B, C_ = V.shape
    n = 2 * E * B
    cls = torch.full((PAD + n + PAD,), -7, dtype=torch.int32, device=DEV)
    out = torch.full((2, PAD + n + PAD), float("nan"), dtype=torch.float64, device=DEV)
    Vd = _dev(V.astype(np.int32))
    rc = lib.bmi_finalize_votes(E, B, C_, ptr(Vd), C.c_void_p(cls.data_ptr() + 4 * PAD), C.c_void_p(out[0].data_ptr() + 8 * PAD),
                                C.c_void_p(out[1].data_ptr() + 8 * PAD), stream())
    torch.cuda.synchronize()
    c, o = cls.cpu().numpy(), out.cpu().numpy()
    assert (c[:PAD] == -7).all() and (c[-PAD:] == -7).all() and np.isnan(o[:, :PAD]).all() and np.isnan(o[:, -PAD:]).all()
    return rc, c[PAD:-PAD].reshape(2, E, B), o[0, PAD:-PAD].reshape(2, E, B), o[1, PAD:-PAD].reshape(2, E, B)


@pytest.mark.parametrize("case", [CASES[0], CASES[3], CASES[4], CASES[5], CASES[7]], ids=case_id)
def test_read_out(case):
    """Classes exactly, ratios bitwise (one float64 division and one subtraction of integers), entropies to 1e-12 relative (the tolerance
    the project's float64 kernels hold against their restatements, tests/test_temperature.py: the device's log against numpy's)."""
    V = reference(case, "none", False)[3].copy()
    E, B, C_ = V.shape[1:]
    rng = np.random.default_rng(case[5])
    V[0, 0, 0] = 0                                                     # no vote cast
    if B > 1:
        V[1, 0, 1] = 0
        V[1, 0, 1, [C_ - 1, 0]] = 7                                    # tied counts: the lowest class
        V[0, E - 1, B - 1] = rng.integers(0, 1000, C_)                 # many classes with votes
    want = vote_readout_numpy(V)
    rc, cls, ratio, ent = run_finalize(V)
    assert rc == _lib.BMI_OK
    assert np.array_equal(cls, want["vote_class"]) and cls[0, 0, 0] == -1
    assert np.array_equal(ratio.view(np.int64), want["variation_ratio"].view(np.int64)) and ratio[0, 0, 0] == 1.0
    print(f"{case}: max relative entropy difference {float(np.abs(ent - want['vote_entropy']).max() / max(want['vote_entropy'].max(), 1e-300)):.2e}")
    np.testing.assert_allclose(ent, want["vote_entropy"], rtol=1e-12, atol=0)
    assert ent[0, 0, 0] == 0.0 and np.isfinite(ent).all() and (ent >= 0).all() and not np.signbit(ent).any()
    if B > 1:
        assert cls[1, 0, 1] == 0 and ratio[1, 0, 1] == 0.5
        np.testing.assert_allclose(ent[1, 0, 1], np.log(2), rtol=1e-12)


MODELS = {"block_exit_c10": dict(dropout_exit=True, dropout="block", dropout_p=0.25, out_dim=10),
          "exit_only_c100": dict(dropout_exit=True, dropout=None, dropout_p=0.25, out_dim=100)}


def _np(r):
    return {k: v.cpu().numpy() for k, v in r.items()}


def _votes(eng, x, T, seed, t_ranges=None):
    B = x.shape[0]
    S, H, Q, QH = eng.new_ensemble_sums(B)
    V = eng.new_vote_counts(B)
    for t0, n in (t_ranges or [(0, T)]):
        eng.accumulate_votes(x, S, H, Q, QH, V, t0, n, seed, 0)
    return S, H, Q, QH, V


@pytest.mark.parametrize("chunk", [None, 2], ids=["chunk_default", "chunk2"])
@pytest.mark.parametrize("dt", ["f16", "f16x2"])
@pytest.mark.parametrize("name", list(MODELS))
def test_engine(name, dt, chunk):
    B, T, seed = 6, 5, 13
    model = synthetic_weights_(build_seeded(ResNet18MCEarlyExit, MODELS[name]), 0).to(DEV).eval()
    x = synthetic_images(B, seed=5).to(DEV)
    eng = MCDEngine(model, DEV, max_batch=B, chunk_samples=chunk, dtype=dt)
    E, Cd = eng.n_exits, eng.out_dim
    if chunk:
        assert eng.chunk_samples == chunk < T
    # the sums are accumulate_ensemble's bits
    S0, H0, Q0, QH0 = eng.new_ensemble_sums(B)
    eng.accumulate_ensemble(x, S0, H0, Q0, QH0, 0, T, seed, 0)
    S, H, Q, QH, V = _votes(eng, x, T, seed)
    assert torch.equal(S, S0) and torch.equal(H, H0) and torch.equal(Q, Q0) and torch.equal(QH, QH0)
    # the stand-alone entry on the same engine's per-sample logits: device against device, no gap condition
    logits = eng.forward_samples(x, T, seed=seed)
    assert torch.equal(V, eng.vote_counts(logits))
    Vn = V.cpu().numpy()
    assert (Vn.sum(-1) == T).all() and np.array_equal(Vn[1, 0], Vn[0, 0])
    assert np.array_equal(Vn[0], vote_counts_numpy(logits.cpu().numpy())[0][0])
    # the split of T into calls adds up exactly
    for ranges in ([(0, 2), (2, 3)], [(0, 1), (1, 1), (2, 3)]):
        assert torch.equal(_votes(eng, x, T, seed, ranges)[4], V), ranges
    # the rows of an image share are the whole batch's rows
    lo = next(o for o in (2, 4) if eng.image_offset_ok(o))
    part = eng.new_ensemble_sums(B - lo)
    Vp = eng.new_vote_counts(B - lo)
    eng.accumulate_votes(x[lo:], *part, Vp, 0, T, seed, 0, image_offset=lo)
    assert torch.equal(Vp, V[:, :, lo:].contiguous())
    # predict_votes: predict_ensemble's dict plus the read-out of these counts
    r, r0 = eng.predict_votes(x, T, seed=seed), eng.predict_ensemble(x, T, seed=seed)
    assert all(torch.equal(r[k], r0[k]) for k in r0) and torch.equal(r["votes"], V[0]) and torch.equal(r["ens_votes"], V[1])
    want = vote_readout_numpy(Vn)
    for pre, kind in (("", 0), ("ens_", 1)):
        assert np.array_equal(r[pre + "vote_class"].cpu().numpy(), want["vote_class"][kind])
        assert np.array_equal(r[pre + "variation_ratio"].cpu().numpy(), want["variation_ratio"][kind])
        np.testing.assert_allclose(r[pre + "vote_entropy"].cpu().numpy(), want["vote_entropy"][kind], rtol=1e-12, atol=0)
    # a map and weights set on the engine: the stand-alone entry given the same parameters
    W = make_weights(E, 3)
    eng.set_ensemble_weights(W)
    Vw = _votes(eng, x, T, seed)[4]
    assert torch.equal(Vw, eng.vote_counts(logits, weights=W)) and torch.equal(Vw[0], V[0])
    for kind in ("tau", "vector", "matrix"):
        cal = make_map(kind, E, Cd, 3)
        eng.set_temperature(cal.get("tau"))
        if kind == "vector":
            eng.set_vector_scaling(cal["scale"], cal["bias"])
        if kind == "matrix":
            eng.set_vector_scaling(None)
            eng.set_matrix_scaling(cal["matrix"], cal["bias"])
        Vc = _votes(eng, x, T, seed)[4]
        assert torch.equal(Vc, eng.vote_counts(logits, weights=W, **cal)), kind
        assert np.array_equal(Vc.cpu().numpy()[0], vote_counts_numpy(logits.cpu().numpy(), **cal)[0][0]), kind
    eng.check_finite()


def test_hipgraph_capture_and_replay():
    """bmi_forward_mcd_votes neither allocates nor synchronises (the scratch belongs to the engine from the warm-up on): a captured
    accumulate_votes + read-out replays on new inputs to the eager bits."""
    model = synthetic_weights_(build_seeded(ResNet18MCEarlyExit, MODELS["block_exit_c10"]), 0).to(DEV).eval()
    B, T, seed = 4, 6, 21
    eng = MCDEngine(model, DEV, max_batch=B, dtype="f16")
    x_static = synthetic_images(B, seed=1).to(DEV)
    S, H, Q, QH = eng.new_ensemble_sums(B)
    V = eng.new_vote_counts(B)
    out_static = {}
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):                      # warm-up on the capture stream (module load, first launches, the scratch)
        eng.accumulate_votes(x_static, S, H, Q, QH, V, 0, T, seed)
        eng.finalize_votes(V)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        S._base.zero_()
        V.zero_()
        eng.accumulate_votes(x_static, S, H, Q, QH, V, 0, T, seed)
        out_static.update(eng.finalize_ensemble(S, H, Q, QH, T))
        out_static.update(eng.finalize_votes(V))
    for s in (2, 3):
        x_new = synthetic_images(B, seed=s).to(DEV)
        x_static.copy_(x_new)
        graph.replay()
        torch.cuda.synchronize()
        got = {k: v.clone() for k, v in out_static.items()}
        want = eng.predict_votes(x_new, T, seed=seed)
        assert set(got) == set(want)
        for k in want:
            assert torch.equal(got[k], want[k]), k
    eng.check_finite()


def test_uncertainty_analysis_with_votes(tmp_path, monkeypatch):
    kw = MODELS["block_exit_c10"]
    m = synthetic_weights_(build_seeded(ResNet18MCEarlyExit, kw), 0).to(DEV).eval()
    m.engine_dtype = "f16"
    B, T, seed = 4, 6, 7
    x, y = synthetic_images(3 * B, seed=3), synthetic_labels(3 * B, 10, seed=4)
    loader = [(x[i * B:(i + 1) * B], y[i * B:(i + 1) * B]) for i in range(3)]
    ua0 = UncertaintyAnalysis(m, loader, gpu=0, mc_passes=T, seed=seed, ensemble=True)
    ua = UncertaintyAnalysis(m, loader, gpu=0, mc_passes=T, seed=seed, votes=True)
    assert ua.ensemble and ua.count_votes and not ua0.count_votes and not hasattr(ua0, "variation_ratio")
    monkeypatch.chdir(tmp_path)
    f0 = np.load(ua0.save("ens"))
    for q in f0.files:                                 # every attribute of the ensemble=True walk keeps its numbers
        assert np.array_equal(getattr(ua, q), getattr(ua0, q)), q
    eng = m.engine(torch.device(DEV), max_batch=B)
    E = eng.n_exits
    for k, (bx, _) in enumerate(loader):
        r = _np(eng.predict_votes(bx.to(DEV), T, seed + k))
        sl = slice(k * B, (k + 1) * B)
        for n in UncertaintyAnalysis.VOTE_KEYS:
            assert np.array_equal(getattr(ua, n)[:, sl], r[n]), n
            assert np.array_equal(getattr(ua, "ensemble_" + n)[:, sl], r["ens_" + n]), n
    assert ua.votes.shape == (E, 3 * B, 10) and ua.votes.dtype == np.int32 and (ua.votes.sum(-1) == T).all()
    assert ua.vote_class.shape == (E, 3 * B) and ua.vote_class.dtype == np.int32 and ua.variation_ratio.shape == (E, 3 * B)
    np.testing.assert_array_equal(ua.mean_variation_ratio, ua.variation_ratio.mean(1))
    np.testing.assert_array_equal(ua.vote_agreement, (ua.vote_class == ua.mean.argmax(-1)).mean(1))
    assert ((0 <= ua.variation_ratio) & (ua.variation_ratio <= 1 - 1 / T + 1e-15)).all()
    assert ((0 <= ua.vote_agreement) & (ua.vote_agreement <= 1)).all()
    s = ua.summary()
    assert [d["mean_variation_ratio"] for d in s] == [float(v) for v in ua.mean_variation_ratio]
    assert [d["vote_agreement"] for d in s] == [float(v) for v in ua.vote_agreement] and "vote_agreement" not in ua0.summary()[0]
    f = np.load(ua.save("votes"))
    new = {"votes", "vote_class", "variation_ratio", "vote_entropy", "mean_variation_ratio", "vote_agreement"}
    new |= {"ensemble_" + n for n in new}
    assert set(f.files) == set(f0.files) | new
    for q in new:
        np.testing.assert_array_equal(f[q], ua._vote_arrays()[q])
