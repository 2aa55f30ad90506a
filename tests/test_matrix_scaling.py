"""-m gpu: matrix scaling — the full [C, C] logit map inside the fused exit head and the exit-ensemble kernel
(bmi_engine_set_matrix_scaling), and the on-device value-and-gradient of its fit (bmi_nll_matrix_scaling_grad).  Off is bit for bit the
engine without one; a diagonal matrix is bit for bit the engine under the same vector scaling on every path (which pins the new
instantiations' arithmetic and reduction order to the tested ones); a permutation matrix permutes the classes (the off-diagonal acts, and
is not transposed); under a real matrix the head's moments are those of the mapped per-sample softmax of the SAME engine's raw logits;
chunking / t-range / image-share invariances and graphs compose with it; the fit kernel equals its numpy restatement and the loader-level
fit lowers the vector fit's NLL."""
import numpy as np
import pytest
import torch

from bayesnn_fpga_amd import _lib
from bayesnn_fpga_amd.engine import BatchesInFlight, MCDEngine
from bayesnn_fpga_amd.synthetic import synthetic_images
from bayesnn_fpga_amd.train.calibration import MatrixScaling, matrix_logits, matrix_z, nll_matrix_numpy
from bayesnn_fpga_amd.train.results_analyzer import FullAnalysis
from bayesnn_fpga_amd.train.uncertainty import decompose_ensemble_logits, decompose_logits, entropy_rows
from tests.test_exit_ensemble import _check_against_host
from tests.test_temperature import BLOCK_10, EXIT_ONLY_10, EXIT_ONLY_100, _model
from tests.test_uncertainty import _invariance_engines, _np, _sums
from tests.test_vector_scaling import _all_paths, _differences

pytestmark = [pytest.mark.gpu, pytest.mark.usefixtures("fp16_engine_default")]
DEV = "cuda:0"
EXIT_ONLY_37 = dict(EXIT_ONLY_10, out_dim=37)                # a partial class tile and an odd C
KWS = {"exit_only_c100": EXIT_ONLY_100, "block_c10": BLOCK_10}       # C = 100: four class tiles, class split, the heads as one pack
KWS3 = dict(KWS, exit_only_c37=EXIT_ONLY_37)
B6, SEED = 6, 3
TS = (40, 33)                # two sample groups plus the join; a second group with one live sample
W_ENS = [1.0, 2.0, 3.0, 4.0]


def _coeffs(E, C, seed=0):
    """The diagonal in [0.4, 2.2] and the bias in [-1, 1] (tests/test_vector_scaling.py's ranges), the off-diagonal U(-1, 1) * 0.3 / sqrt(C),
    not symmetric: z keeps the range the project's softmax tolerances were granted for."""
    rng = np.random.default_rng(300 + seed)
    M = rng.uniform(-1.0, 1.0, (E, C, C)) * 0.3 / np.sqrt(C)
    M[:, np.arange(C), np.arange(C)] = rng.uniform(0.4, 2.2, (E, C))
    return M.astype(np.float32), rng.uniform(-1.0, 1.0, (E, C)).astype(np.float32)


def _diag(a):
    E, C = a.shape
    M = np.zeros((E, C, C), np.float32)
    M[:, np.arange(C), np.arange(C)] = a
    return M


def _engine(m, dt, head_batch, B=B6):
    eng = MCDEngine(m, DEV, max_batch=B, dtype=dt)
    eng.set_option("head_batch", head_batch)
    return eng


# ---- 1. off is off ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("head_batch", [0, 1])
@pytest.mark.parametrize("dt", ["f16", "f16x2"])
def test_off_is_off(dt, head_batch):
    """None, and set-then-clear, give S / SH / the ensemble sums torch.equal to an engine that never had a map; with a matrix set S1, SH and
    Q differ and SL is torch.equal."""
    for kw in KWS.values():
        m = _model(kw)
        x = synthetic_images(B6, seed=5).to(DEV)
        ref, eng = _engine(m, dt, head_batch), _engine(m, dt, head_batch)
        T = TS[0]

        def run(e):
            S, H, Q, QH = e.new_ensemble_sums(B6)
            e.accumulate_ensemble(x, S, H, Q, QH, 0, T, SEED)
            return S, H, Q, QH
        want = run(ref)
        eng.set_matrix_scaling(None)
        assert eng.matrix_scaling is None
        assert all(torch.equal(a, b) for a, b in zip(run(eng), want))
        M, b = _coeffs(eng.n_exits, eng.out_dim)
        eng.set_matrix_scaling(M, b)
        assert np.array_equal(eng.matrix_scaling[0], M) and np.array_equal(eng.matrix_scaling[1], b)
        S, H, Q, QH = run(eng)
        assert not torch.equal(S[0], want[0][0]) and not torch.equal(H, want[1]) and not torch.equal(Q, want[2])
        assert torch.equal(S[2], want[0][2])                                    # SL stays the raw logit sum
        eng.set_matrix_scaling(None)
        assert all(torch.equal(a, b) for a, b in zip(run(eng), want))


# ---- 2. anchored to vector scaling, bit for bit -----------------------------------------------------------------------------------
@pytest.mark.parametrize("head_batch", [0, 1])
@pytest.mark.parametrize("dt", ["f16", "f16x2"])
@pytest.mark.parametrize("name", KWS)
def test_a_diagonal_matrix_is_the_vector_scaled_engine_on_every_path(name, dt, head_batch):
    """M = diag(a) with bias b for a real per-class (a, b) equals the engine under set_vector_scaling(a, b), torch.equal on every entry of
    _all_paths — the moment and entropy sums, the ensemble read-out unweighted and weighted, adaptive sampling under both stop_on, staged
    exit under both rules: the off-diagonal products are +-0 and fl(fl(a l_c) + b) is vector scaling's number.  Every entry that differs is
    printed before the assertion; a non-diagonal matrix then differs, so the comparison is not vacuous."""
    m = _model(KWS[name])
    x = synthetic_images(B6, seed=5).to(DEV)
    ref, eng = _engine(m, dt, head_batch), _engine(m, dt, head_batch)
    E, C = eng.n_exits, eng.out_dim
    rng = np.random.default_rng(100)
    a, b = rng.uniform(0.4, 2.2, (E, C)).astype(np.float32), rng.uniform(-1.0, 1.0, (E, C)).astype(np.float32)
    ref.set_vector_scaling(a, b)
    eng.set_matrix_scaling(_diag(a), b)
    bad = []
    for T in TS:
        got = _all_paths(eng, x, T)
        bad += [(T, k, d) for k, d in _differences(got, _all_paths(ref, x, T))]
    for T, k, d in bad:
        print(f"{name} {dt} hb{head_batch} T={T}: {k} differs" + ("" if d is None else f", largest absolute difference {d:.3e}"))
    eng.set_matrix_scaling(*_coeffs(E, C))
    assert not torch.equal(_all_paths(eng, x, TS[1])["S"][0], got["S"][0])       # (the comparison above is not vacuous)
    assert not bad, bad


# ---- 3. the off-diagonal acts, and is not transposed ------------------------------------------------------------------------------
@pytest.mark.parametrize("head_batch", [0, 1])
@pytest.mark.parametrize("name", KWS3)
def test_a_permutation_matrix_permutes_the_classes(name, head_batch):
    """With M[c][pi(c)] = 1 and a zero bias z_c = l_pi(c) exactly, so mean[..., c] is the unscaled engine's mean[..., pi(c)] within 1e-5, the
    project's head-softmax figure (the class sum's order changes, so not bit-equal); logit_mean is torch.equal to the unscaled run."""
    m = _model(KWS3[name])
    x = synthetic_images(B6, seed=5).to(DEV)
    eng = _engine(m, "f16x2", head_batch)
    C = eng.out_dim
    pi = np.random.default_rng(C).permutation(C)
    assert not np.array_equal(pi, np.argsort(pi))            # (not an involution: a transposed matrix is caught)
    M = np.zeros((C, C), np.float32)
    M[np.arange(C), pi] = 1.0
    for T in TS:
        off = eng.predict(x, T, seed=SEED)
        eng.set_matrix_scaling(M)
        r = eng.predict(x, T, seed=SEED)
        eng.set_matrix_scaling(None)
        err = float((r["mean"] - off["mean"][..., torch.from_numpy(pi).to(DEV)]).abs().max())
        err_t = float((r["mean"] - off["mean"][..., torch.from_numpy(np.argsort(pi)).to(DEV)]).abs().max())
        print(f"{name} hb{head_batch} T={T}: |mean - permuted| {err:.2e} (transposed: {err_t:.2e})")
        assert err <= 1e-5 and err_t > err
        assert torch.equal(r["logit_mean"], off["logit_mean"])


# ---- 4. self-consistency under a real matrix --------------------------------------------------------------------------------------
@pytest.mark.parametrize("head_batch", [0, 1])
@pytest.mark.parametrize("dt", ["f16", "f16x2"])
@pytest.mark.parametrize("name", KWS3)
def test_self_consistency(name, dt, head_batch):
    """mean / var against matrix_logits of the SAME engine's forward_samples logits: 1e-5 / 4e-5, the figures tests/test_temperature.py
    grants the head's fp32 softmax (the restatement reproduces z exactly, so nothing else enters); logit_mean and forward_samples are
    bit-equal to the unscaled run; exp_entropy within 1e-5 of the host decomposition; predict_ensemble against
    decompose_ensemble_logits(raw, matrix=, bias=) within tests/test_exit_ensemble.py's tolerances, unweighted and weighted;
    ensemble_moments on the same logits gives predict_ensemble's ens_mean bit for bit."""
    m = _model(KWS3[name])
    x = synthetic_images(B6, seed=5).to(DEV)
    eng = _engine(m, dt, head_batch)
    M, b = _coeffs(eng.n_exits, eng.out_dim)
    for T in TS:
        off = eng.predict(x, T, seed=SEED)
        logits_off = eng.forward_samples(x, T, seed=SEED, cnt0=0)
        raw = logits_off.cpu().numpy()
        eng.set_matrix_scaling(M, b)
        r = eng.predict(x, T, seed=SEED)
        eng.check_finite()
        mean, var = matrix_logits(raw, M, b)
        e_mean = float(np.abs(r["mean"].cpu().numpy() - mean).max())
        e_var = float(np.abs(r["var"].cpu().numpy() - var).max())
        print(f"{name} {dt} hb{head_batch} T={T}: |mean - mapped| {e_mean:.2e}, |var - mapped| {e_var:.2e}")
        assert e_mean <= 1e-5 and e_var <= 4e-5, (e_mean, e_var)
        assert torch.equal(r["logit_mean"], off["logit_mean"])
        assert torch.equal(eng.forward_samples(x, T, seed=SEED, cnt0=0), logits_off)
        assert not torch.equal(r["mean"], off["mean"])
        u = _np(eng.predict_uncertainty(x, T, seed=SEED, cnt0=0))
        np.testing.assert_allclose(u["exp_entropy"], decompose_logits(matrix_z(raw, M, b))["exp_entropy"], rtol=0, atol=1e-5)
        np.testing.assert_allclose(u["pred_entropy"], entropy_rows(u["mean"]), rtol=0, atol=1e-9)
        ens = eng.predict_ensemble(x, T, seed=SEED)
        _check_against_host(_np(ens), decompose_ensemble_logits(raw, matrix=M, bias=b), f"{name} mapped")
        eng.set_ensemble_weights(W_ENS)
        _check_against_host(_np(eng.predict_ensemble(x, T, seed=SEED)), decompose_ensemble_logits(raw, weights=W_ENS, matrix=M, bias=b),
                            f"{name} mapped, weighted")
        eng.set_ensemble_weights(None)
        mom = eng.ensemble_moments(logits_off, matrix=M, bias=b)          # the stand-alone entry on the same logits: the engine's own sums
        assert torch.equal(mom["ens_mean"], ens["ens_mean"])
        eng.set_matrix_scaling(None)


# ---- 5. invariances ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", KWS)
def test_invariances_under_matrix_scaling(name):
    """tests/test_vector_scaling.py::test_invariances_under_vector_scaling with a matrix set on the model (every engine built from it
    inherits it): 70 samples in one call against launches of at most 32, T split in t-ranges, image shares through image_offset — rtol
    1e-12 on S and H; head_batch 1 against 0 and two identical runs bit for bit."""
    kw = KWS[name]
    B, T, seed = 8, 70, 11
    model = _model(kw)
    M, b = _coeffs(4, kw["out_dim"], seed=1)
    model.set_exit_matrix_scaling(M, b)
    x = synthetic_images(B, seed=77).to(DEV)
    e_def, e32 = _invariance_engines(model, B)
    assert np.array_equal(e_def.matrix_scaling[0], M) and np.array_equal(e32.matrix_scaling[1], b) and e_def.chunk_samples >= T
    S, H = _sums(e_def, x, T, seed)
    runs = [_sums(e_def, x, T, seed, t_ranges=[(0, 32), (32, 32), (64, T - 64)]), _sums(e_def, x, T, seed, t_ranges=[(0, 29), (29, T - 29)]),
            _sums(e_def, x, T, seed, shares=[(0, 4), (4, 8)])]
    if kw["dropout"] is None:        # (with convs in the suffix two plans pick different fp16 conv kernels: tests/test_uncertainty.py)
        runs.append(_sums(e32, x, T, seed))
    for S2, H2 in runs:
        np.testing.assert_allclose(H2, H, rtol=1e-12, atol=0)
        np.testing.assert_allclose(S2, S, rtol=1e-12, atol=1e-12)
    S1, H1 = _sums(e_def, x, T, seed)
    assert np.array_equal(S1, S) and np.array_equal(H1, H)
    e_def.set_matrix_scaling(None)
    S_off, _ = _sums(e_def, x, T, seed)
    assert not np.array_equal(S_off[0], S[0]) and np.array_equal(S_off[2], S[2])
    e_def.set_matrix_scaling(M, b)
    e_def.set_option("head_batch", 0)
    S0, H0 = _sums(e_def, x, T, seed)
    assert np.array_equal(S0, S) and np.array_equal(H0, H)


# ---- 6. graphs --------------------------------------------------------------------------------------------------------------------
def test_predict_graphed_after_set_matrix_scaling_equals_eager():
    B, T, seed = 8, 4, 9
    m = _model(EXIT_ONLY_10)
    x = synthetic_images(B, seed=12).to(DEV)
    pipe = BatchesInFlight(m, DEV, n=1, max_batch=B, dtype="f16")

    def graphed():
        out = pipe.predict_graphed(x, T, seed)
        pipe.synchronize()
        return {k: v.clone() for k, v in out.items()}
    r0, r0b = graphed(), graphed()                                                     # the capture, then a replay of it
    assert all(torch.equal(r0[k], r0b[k]) for k in r0)
    pipe.set_matrix_scaling(*_coeffs(4, 10))
    assert not hasattr(pipe, "_graphs")
    for _ in range(2):                                                                 # capture, then replay
        r1 = graphed()
        eager = pipe.engines[0].predict(x, T, seed=seed)
        torch.cuda.synchronize()
        assert all(torch.equal(r1[k], eager[k]) for k in eager)
        assert not torch.equal(r1["mean"], r0["mean"]) and torch.equal(r1["logit_mean"], r0["logit_mean"])
    pipe.close()


# ---- 7. the fit kernel ------------------------------------------------------------------------------------------------------------
def _staging_limit(C):
    """Samples one workgroup of bmi_nll_matrix_scaling_grad stages at a time: 64 for C = 10 and 37, 34 for C = 100; beyond it the kernel runs
    in chunks of samples."""
    return min(_lib.NLL_MAT_ROWS, _lib.NLL_MAT_SLAB // (C | 1))


@pytest.mark.parametrize("gain", [None, 24.0], ids=["ordinary", "x24"])
@pytest.mark.parametrize("C", [10, 37, 100])
def test_nll_matrix_grad_equals_its_numpy_restatement(C, gain):
    """nll_matrix_grad against nll_matrix_numpy on the device's own logits, (T, B) in {(1, 1), (10, 7), (33, 5)} and a T on each side of the
    kernel's staging limit, ordinary and x24 logits: the value within 1e-9 relative, the gradients within 1e-9 * max(1, max |l|) — the
    bounds of tests/test_vector_scaling.py: the terms are the same count, each carries one factor |l|, and z is summed in the same order on
    both sides.  The columns of g_matrix sum to 0 within the same bound (the softmax gauge).  Accumulating two batches equals numpy on the
    concatenation to rtol 1e-12; two identical calls are torch.equal."""
    assert [_staging_limit(c) for c in (10, 37, 100)] == [64, 64, 34]
    lim = _staging_limit(C)
    m = _model(dict(EXIT_ONLY_10, out_dim=C), gain=gain)
    eng = m.engine(torch.device(DEV), max_batch=7, dtype="f16x2")
    full = eng.forward_samples(synthetic_images(7, seed=41).to(DEV), lim + 1, seed=17)
    E = full.shape[1]
    rng = np.random.default_rng(C)
    labels_all = rng.integers(0, C, 7)
    M, b = (v.astype(np.float64) for v in _coeffs(E, C, seed=2))
    lmax = float(full.abs().max())
    bound = 1e-9 * max(1.0, lmax)
    print(f"C {C} gain {gain}: max |logit| {lmax:.0f}, staging limit {lim}")
    for T, B in ((1, 1), (10, 7), (33, 5), (lim, 3), (lim + 1, 3)):
        logits = full[:T, :, :B].contiguous()
        y = torch.from_numpy(labels_all[:B])
        got = eng.nll_matrix_grad(logits, y, M, b)
        again = eng.nll_matrix_grad(logits, y, M, b)
        assert all(torch.equal(p, q) for p, q in zip(got, again))
        f, gM, gb = (t.cpu().numpy() for t in got)
        rf, rgM, rgb = nll_matrix_numpy(logits.cpu().numpy(), labels_all[:B], M, b)
        assert np.isfinite(f).all() and np.isfinite(gM).all() and np.isfinite(gb).all()
        e_f = float((np.abs(f - rf) / np.where(rf == 0, 1.0, np.abs(rf))).max())     # (x24, one image: both sides can be exactly 0)
        e_g = max(float(np.abs(gM - rgM).max()), float(np.abs(gb - rgb).max()))
        e_col = float(np.abs(gM.sum(1)).max())
        print(f"  T {T} B {B}: value {e_f:.2e} relative, gradients {e_g:.2e} absolute, column sums {e_col:.2e} (bound {bound:.2e})")
        assert e_f <= 1e-9, (T, B, e_f)
        assert e_g <= bound, (T, B, e_g)
        assert e_col <= bound, (T, B, e_col)
    # two batches accumulated into one triple = numpy on the concatenation
    p, q = full[:10, :, :3].contiguous(), full[:10, :, 3:7].contiguous()
    out = eng.nll_matrix_grad(p, torch.from_numpy(labels_all[:3]), M, b)
    out = eng.nll_matrix_grad(q, torch.from_numpy(labels_all[3:7]), M, b, out=out)
    ref = nll_matrix_numpy(full[:10].cpu().numpy(), labels_all, M, b)
    for g_, r_ in zip(out, ref):
        np.testing.assert_allclose(g_.cpu().numpy(), r_, rtol=1e-12, atol=1e-12 * max(1.0, lmax))


# ---- 8. the fit, end to end -------------------------------------------------------------------------------------------------------
def test_matrix_scaling_fit_end_to_end(tmp_path, monkeypatch):
    """MatrixScaling over a three-batch loader of 8 images (T = 10, C = 100, f16x2) with teacher labels drawn from softmax(M* mean logits),
    M* banded and not diagonal; off_diag_l2 = 1, bias_l2 = 0, max_iter = 12: nll_after <= nll_start (the vector fit's NLL) at every exit and
    below it at some; nll_matrix_numpy at the returned float32 parameters on host copies of the logits equals nll_after to rtol 1e-9;
    after apply() the model has neither a temperature nor a vector scaling and engines / FullAnalysis run under the matrix; save()
    round-trips; a refit gives identical arrays; select over (0.1, 10.0) with the third batch as hold-out returns one row per candidate
    and keeps the one with the lowest hold-out NLL."""
    C, Bb, T, seed = 100, 8, 10, 5
    m = _model(EXIT_ONLY_100)
    m.engine_dtype = "f16x2"
    x = synthetic_images(3 * Bb, seed=31)
    eng = m.engine(torch.device(DEV), max_batch=Bb)
    raw = np.concatenate([eng.forward_samples(x[k * Bb:(k + 1) * Bb].to(DEV), T, seed=seed + k).cpu().numpy() for k in range(3)], axis=2)
    rng = np.random.default_rng(7)
    Ms = np.eye(C) * 1.5
    for c in range(C):
        Ms[c, (c + 1) % C], Ms[c, (c - 1) % C] = 0.9, -0.4
    z = raw.mean(0)[-1].astype(np.float64) @ Ms.T                                # [N, C]
    p = np.exp(z - z.max(-1, keepdims=True))
    labels = np.array([rng.choice(C, p=q / q.sum()) for q in p])
    y = torch.from_numpy(labels)
    loader = [(x[k * Bb:(k + 1) * Bb], y[k * Bb:(k + 1) * Bb]) for k in range(3)]
    m.set_exit_vector_scaling(np.full(C, 0.5))                                   # (apply() has something to clear)
    ms = MatrixScaling(m, loader, gpu=0, mc_passes=T, seed=seed)
    r = ms.fit(off_diag_l2=1.0, bias_l2=0.0, max_iter=12)
    print(f"fit: nll {r['nll_start']} -> {r['nll_after']}, penalty {r['penalty']}, iterations {r['iterations']}, |g| {r['grad_norm']}")
    assert r["n"] == 3 * Bb and r["matrix"].dtype == r["bias"].dtype == np.float32
    assert r["matrix"].shape == (4, C, C) and r["bias"].shape == r["scale0"].shape == r["bias0"].shape == (4, C)
    assert (r["nll_after"] <= r["nll_start"]).all() and (r["nll_after"] < r["nll_start"]).any()
    host = nll_matrix_numpy(raw, labels, r["matrix"].astype(np.float64), r["bias"].astype(np.float64))[0]
    np.testing.assert_allclose(r["nll_after"], host, rtol=1e-9, atol=0)
    M, b = ms.apply()
    assert m.exit_temperature is None and m.exit_vector_scaling is None and np.array_equal(M, r["matrix"]) and np.array_equal(b, r["bias"])
    eng = m.engine(torch.device(DEV), max_batch=Bb)
    assert np.array_equal(eng.matrix_scaling[0], r["matrix"]) and eng.temperature == [1.0] * 4 and eng.vector_scaling is None
    fa = FullAnalysis(m, loader, gpu=0, mc_dropout=True, mc_passes=T, seed=seed, macro_batches=1)
    want = np.concatenate([eng.predict(xb.to(DEV), T, seed=seed + k)["mean"].cpu().numpy() for k, (xb, _) in enumerate(loader)], axis=1)
    np.testing.assert_allclose(fa.preds, want, rtol=0, atol=1e-12)
    mean, _ = matrix_logits(raw, r["matrix"], r["bias"])
    assert float(np.abs(want - mean).max()) <= 1e-5
    monkeypatch.chdir(tmp_path)
    saved = np.load(ms.save("t"))
    assert np.array_equal(saved["matrix"], r["matrix"]) and np.array_equal(saved["bias"], r["bias"]) and np.array_equal(saved["nll_after"], r["nll_after"])
    r2 = MatrixScaling(m, loader, gpu=0, mc_passes=T, seed=seed).fit(off_diag_l2=1.0, max_iter=12)      # raw logits do not depend on the map set
    assert np.array_equal(r2["matrix"], r["matrix"]) and np.array_equal(r2["bias"], r["bias"]) and np.array_equal(r2["nll_after"], r["nll_after"])
    sel = MatrixScaling(m, loader[:2], gpu=0, mc_passes=T, seed=seed)
    table = sel.select(loader[2:], off_diag_l2=(0.1, 10.0), max_iter=12)
    assert [row["off_diag_l2"] for row in table] == [0.1, 10.0] and sum(row["selected"] for row in table) == 1
    best = min(range(2), key=lambda i: table[i]["total_holdout"])
    assert table[best]["selected"] and sel.selected == best and np.array_equal(sel.result["nll_after"], table[best]["nll_after"])
    for row in table:
        print(f"select: off_diag_l2 {row['off_diag_l2']}: validation {row['nll_after']}, hold-out {row['nll_holdout']}")
        assert row["nll_holdout"].shape == (4,) and np.isfinite(row["nll_holdout"]).all()


# ---- 9. ABI errors ----------------------------------------------------------------------------------------------------------------
def test_abi_errors_on_a_live_engine():
    m = _model(EXIT_ONLY_10)
    eng = MCDEngine(m, DEV, max_batch=4)
    E, C = eng.n_exits, eng.out_dim
    M, b = _coeffs(E, C)
    eng.set_temperature(2.0)
    with pytest.raises(ValueError):
        eng.set_matrix_scaling(M, b)
    eng.set_temperature(None)
    eng.set_vector_scaling(np.ones(C))
    with pytest.raises(ValueError):
        eng.set_matrix_scaling(M, b)
    eng.set_vector_scaling(None)
    eng.set_matrix_scaling(M, b)
    with pytest.raises(ValueError):
        eng.set_temperature(2.0)
    with pytest.raises(ValueError):
        eng.set_vector_scaling(np.ones(C))
    eng.set_temperature(1.0)                                                     # all ones is off: allowed
    # a scratch too small: BMI_ERR_NOMEM, nothing written
    T, B = 3, 4
    lib = eng.lib
    logits = eng.forward_samples(synthetic_images(B, seed=1).to(DEV), T, seed=0)
    y = torch.zeros(B, dtype=torch.int32, device=DEV)
    M64, b64 = torch.from_numpy(M).to(DEV).double(), torch.from_numpy(b).to(DEV).double()
    out = [torch.zeros(E, dtype=torch.float64, device=DEV), torch.zeros(E, C, C, dtype=torch.float64, device=DEV),
           torch.zeros(E, C, dtype=torch.float64, device=DEV)]
    need = int(lib.bmi_nll_matrix_scratch_bytes(E, B, C))
    assert need == E * B * (C * C + C + 1) * 8
    scratch = torch.zeros(need, dtype=torch.uint8, device=DEV)
    rc = lib.bmi_nll_matrix_scaling_grad(logits.data_ptr(), T, E, B, C, y.data_ptr(), M64.data_ptr(), b64.data_ptr(), out[0].data_ptr(),
                                         out[1].data_ptr(), out[2].data_ptr(), scratch.data_ptr(), need - 1, None)
    torch.cuda.synchronize()
    assert rc == -12 and not any(bool(o.any()) for o in out) and not bool(scratch.any())
