"""-m gpu: vector scaling — the per-class scale and bias inside the fused exit head and the exit-ensemble kernel
(bmi_engine_set_vector_scaling), and the on-device value-and-gradient of its fit (bmi_nll_vector_scaling_grad).  Off is bit for bit the
engine without one; scale = 1 / tau with a zero bias is bit for bit the tempered engine on every path (which pins the new instantiations'
reduction order to the existing ones); under a real per-class scaling the head's moments are those of the scaled per-sample softmax of the
SAME engine's raw logits; chunking / t-range / image-share invariances and graphs compose with it; the fit kernel equals its numpy
restatement and the loader-level fit lowers the scalar fit's NLL."""
import numpy as np
import pytest
import torch

from bayesnn_fpga_amd import _lib
from bayesnn_fpga_amd.engine import BatchesInFlight, MCDEngine
from bayesnn_fpga_amd.synthetic import synthetic_images
from bayesnn_fpga_amd.train.calibration import VectorScaling, _inv32, nll_vector_numpy, scale_logits
from bayesnn_fpga_amd.train.results_analyzer import FullAnalysis
from bayesnn_fpga_amd.train.uncertainty import decompose_ensemble_logits, decompose_logits, entropy_rows
from tests.test_exit_ensemble import _check_against_host
from tests.test_temperature import BLOCK_10, EXIT_ONLY_10, EXIT_ONLY_100, _model
from tests.test_uncertainty import _invariance_engines, _np, _sums

pytestmark = [pytest.mark.gpu, pytest.mark.usefixtures("fp16_engine_default")]
DEV = "cuda:0"
KWS = {"exit_only_c100": EXIT_ONLY_100, "block_c10": BLOCK_10}       # C = 100: four class tiles, class split, the heads as one pack
B6, SEED = 6, 3
TS = (40, 33)                # two sample groups plus the join; a second group with one live sample
W_ENS = [1.0, 2.0, 3.0, 4.0]


def _coeffs(E, C, seed=0):
    """Scales in [0.4, 2.2] (the range of 1 / tau tests/test_temperature.py uses), biases in [-1, 1], distinct per exit and class."""
    rng = np.random.default_rng(100 + seed)
    return rng.uniform(0.4, 2.2, (E, C)).astype(np.float32), rng.uniform(-1.0, 1.0, (E, C)).astype(np.float32)


def _engine(m, dt, head_batch, B=B6):
    eng = MCDEngine(m, DEV, max_batch=B, dtype=dt)
    eng.set_option("head_batch", head_batch)
    return eng


def _differences(a, b, prefix=""):
    """The entries of two result dicts that do not agree bit for bit (tensors, nested dicts) / exactly (host values): [(name, largest
    absolute difference)]."""
    assert a.keys() == b.keys()
    out = []
    for k in a:
        if isinstance(a[k], torch.Tensor):
            if not torch.equal(a[k], b[k]):
                out.append((prefix + k, float((a[k].double() - b[k].double()).abs().max())))
        elif isinstance(a[k], dict):
            out += _differences(a[k], b[k], f"{prefix}{k}/")
        elif a[k] != b[k]:
            out.append((prefix + k, None))
    return out


def _all_paths(eng, x, T):
    """Everything the issue's anchor test compares, as one dict of results: the entropy walk's sums, the ensemble read-out unweighted and
    weighted, adaptive sampling under both stop_on, staged early exit under both rules' predictors."""
    S, H = eng.new_uncertainty_sums(x.shape[0])
    eng.accumulate_uncertainty(x, S, H, 0, T, SEED)
    out = dict(S=S, H=H, ens=eng.predict_ensemble(x, T, seed=SEED))
    eng.set_ensemble_weights(W_ENS)
    out["ens_w"] = eng.predict_ensemble(x, T, seed=SEED)
    eng.set_ensemble_weights(None)
    full = eng.finalize(S.clone(), T)
    sem = float(torch.sqrt(full["var"][-1].max(-1).values / (T / 2)).median())
    for stop_on in ("exit", "ensemble"):
        out["adaptive_" + stop_on] = eng.predict_adaptive(x, T, sem, rule="sem", t_step=8, seed=SEED, ensemble=True, stop_on=stop_on)
    thr = float(full["mean"][1].max(-1).values.median())
    if T <= eng.chunk_samples:
        for ens in (False, True):
            out[f"early_{ens}"] = eng.predict_early_exit(x, T, thr, seed=SEED, ensemble=ens, ensemble_readout=True)
    return out


# ---- 1. off is off ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("head_batch", [0, 1])
@pytest.mark.parametrize("dt", ["f16", "f16x2"])
def test_off_is_off(dt, head_batch):
    """None, and set-then-clear, give S / SH / the ensemble sums torch.equal to an engine that never had a scaling."""
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
        eng.set_vector_scaling(None)
        assert eng.vector_scaling is None
        assert all(torch.equal(a, b) for a, b in zip(run(eng), want))
        a, b = _coeffs(eng.n_exits, eng.out_dim)
        eng.set_vector_scaling(a, b)
        assert np.array_equal(eng.vector_scaling[0], a) and np.array_equal(eng.vector_scaling[1], b)
        S, H, Q, QH = run(eng)
        assert not torch.equal(S[0], want[0][0]) and not torch.equal(H, want[1]) and not torch.equal(Q, want[2])
        assert torch.equal(S[2], want[0][2])                                    # SL stays the raw logit sum
        eng.set_vector_scaling(None)
        assert all(torch.equal(a, b) for a, b in zip(run(eng), want))


# ---- 2. anchored to the tested paths, bit for bit ---------------------------------------------------------------------------------
ANCHORS = {"ones": None, "uniform_0.5": [0.5] * 4, "distinct": [0.7, 1.0, 1.9, 3.1]}


@pytest.mark.parametrize("tag", ANCHORS)
@pytest.mark.parametrize("head_batch", [0, 1])
@pytest.mark.parametrize("dt", ["f16", "f16x2"])
@pytest.mark.parametrize("name", KWS)
def test_anchored_to_the_unscaled_and_the_tempered_engine(name, dt, head_batch, tag):
    """scale = ones, bias = zeros through the vector kernels equals the unscaled engine (fl(fl(l * 1) + 0) = l), and scale = float32(1 / tau)
    for every class with a zero bias equals the engine under set_temperature(tau) (fl(fl(l * inv) + 0) = fl(l * inv)), torch.equal on
    every result of every path: the moment and entropy sums, the ensemble read-out unweighted and weighted, adaptive sampling's t_used /
    converged under both stop_on, staged early exit's exits and sums.  Every entry that differs is printed before the assertion.

    The "distinct" case is the one that sees a product fused into the subtraction of the max (a power-of-two factor is exact either way): it
    found the tempered kernels doing so — S1 / S2 off by up to 4.8e-7 in sums over 40 samples, SH by up to 7.8e-7, the ensemble sums and the
    decisions equal — and both scaled states now form their products under fp contract(off) (profiles/vector_scaling.md)."""
    m = _model(KWS[name])
    x = synthetic_images(B6, seed=5).to(DEV)
    ref, eng = _engine(m, dt, head_batch), _engine(m, dt, head_batch)
    E, C = eng.n_exits, eng.out_dim
    tau = ANCHORS[tag]
    ref.set_temperature(tau)
    inv = np.ones(E, np.float32) if tau is None else _inv32(tau)
    eng.set_vector_scaling(np.repeat(inv[:, None], C, axis=1), np.zeros((E, C)))
    bad = []
    for T in TS:
        got = _all_paths(eng, x, T)
        bad += [(T, k, d) for k, d in _differences(got, _all_paths(ref, x, T))]
    for T, k, d in bad:
        print(f"{name} {dt} hb{head_batch} {tag} T={T}: {k} differs" + ("" if d is None else f", largest absolute difference {d:.3e}"))
    ref.set_temperature(None)
    eng.set_vector_scaling(*_coeffs(E, C))
    assert not torch.equal(_all_paths(eng, x, TS[1])["S"][0], got["S"][0])       # (the comparison above is not vacuous)
    assert not bad, bad


# ---- 3. self-consistency under a real per-class scaling ---------------------------------------------------------------------------
@pytest.mark.parametrize("head_batch", [0, 1])
@pytest.mark.parametrize("dt", ["f16", "f16x2"])
@pytest.mark.parametrize("name", KWS)
def test_self_consistency(name, dt, head_batch):
    """mean / var against scale_logits of the SAME engine's forward_samples logits: 1e-5 / 4e-5, the figures tests/test_temperature.py
    grants the head's fp32 softmax (the restatement reproduces z exactly, so nothing else enters); logit_mean and forward_samples are
    bit-equal to the unscaled run; exp_entropy within 1e-5 of the host decomposition; predict_ensemble against
    decompose_ensemble_logits(raw, scale=, bias=) within tests/test_exit_ensemble.py's tolerances, unweighted and weighted."""
    m = _model(KWS[name])
    x = synthetic_images(B6, seed=5).to(DEV)
    eng = _engine(m, dt, head_batch)
    a, b = _coeffs(eng.n_exits, eng.out_dim)
    for T in TS:
        off = eng.predict(x, T, seed=SEED)
        logits_off = eng.forward_samples(x, T, seed=SEED, cnt0=0)
        raw = logits_off.cpu().numpy()
        eng.set_vector_scaling(a, b)
        r = eng.predict(x, T, seed=SEED)
        eng.check_finite()
        mean, var = scale_logits(raw, a, b)
        e_mean = float(np.abs(r["mean"].cpu().numpy() - mean).max())
        e_var = float(np.abs(r["var"].cpu().numpy() - var).max())
        print(f"{name} {dt} hb{head_batch} T={T}: |mean - scaled| {e_mean:.2e}, |var - scaled| {e_var:.2e}")
        assert e_mean <= 1e-5 and e_var <= 4e-5, (e_mean, e_var)
        assert torch.equal(r["logit_mean"], off["logit_mean"])
        assert torch.equal(eng.forward_samples(x, T, seed=SEED, cnt0=0), logits_off)
        assert not torch.equal(r["mean"], off["mean"])
        u = _np(eng.predict_uncertainty(x, T, seed=SEED, cnt0=0))
        z = ((raw * a[None, :, None, :]).astype(np.float32) + b[None, :, None, :]).astype(np.float32)
        np.testing.assert_allclose(u["exp_entropy"], decompose_logits(z)["exp_entropy"], rtol=0, atol=1e-5)
        np.testing.assert_allclose(u["pred_entropy"], entropy_rows(u["mean"]), rtol=0, atol=1e-9)
        _check_against_host(_np(eng.predict_ensemble(x, T, seed=SEED)), decompose_ensemble_logits(raw, scale=a, bias=b), f"{name} scaled")
        eng.set_ensemble_weights(W_ENS)
        _check_against_host(_np(eng.predict_ensemble(x, T, seed=SEED)), decompose_ensemble_logits(raw, weights=W_ENS, scale=a, bias=b),
                            f"{name} scaled, weighted")
        eng.set_ensemble_weights(None)
        # the stand-alone entry on the same logits: the engine's own sums
        mom = eng.ensemble_moments(logits_off, scale=a, bias=b)
        assert torch.equal(mom["ens_mean"], eng.predict_ensemble(x, T, seed=SEED)["ens_mean"])
        eng.set_vector_scaling(None)


# ---- 4. invariances ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", KWS)
def test_invariances_under_vector_scaling(name):
    """tests/test_temperature.py's invariance assertions with a vector scaling set on the model (every engine built from it inherits it):
    70 samples in one call against launches of at most 32, T split in t-ranges, image shares through image_offset — rtol 1e-12 on S and H;
    head_batch 1 against 0 and two identical runs bit for bit."""
    kw = KWS[name]
    B, T, seed = 8, 70, 11
    model = _model(kw)
    a, b = _coeffs(4, kw["out_dim"], seed=1)
    model.set_exit_vector_scaling(a, b)
    x = synthetic_images(B, seed=77).to(DEV)
    e_def, e32 = _invariance_engines(model, B)
    assert np.array_equal(e_def.vector_scaling[0], a) and np.array_equal(e32.vector_scaling[1], b) and e_def.chunk_samples >= T
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
    e_def.set_vector_scaling(None)
    S_off, _ = _sums(e_def, x, T, seed)
    assert not np.array_equal(S_off[0], S[0]) and np.array_equal(S_off[2], S[2])
    e_def.set_vector_scaling(a, b)
    e_def.set_option("head_batch", 0)
    S0, H0 = _sums(e_def, x, T, seed)
    assert np.array_equal(S0, S) and np.array_equal(H0, H)


# ---- 5. graphs --------------------------------------------------------------------------------------------------------------------
def test_predict_graphed_after_set_vector_scaling_equals_eager():
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
    pipe.set_vector_scaling(*_coeffs(4, 10))
    assert not hasattr(pipe, "_graphs")
    for _ in range(2):                                                                 # capture, then replay
        r1 = graphed()
        eager = pipe.engines[0].predict(x, T, seed=seed)
        torch.cuda.synchronize()
        assert all(torch.equal(r1[k], eager[k]) for k in eager)
        assert not torch.equal(r1["mean"], r0["mean"]) and torch.equal(r1["logit_mean"], r0["logit_mean"])
    pipe.close()


# ---- 6. the fit kernel ------------------------------------------------------------------------------------------------------------
def _staging_limit(C):
    """Samples one workgroup of bmi_nll_vector_scaling_grad stages at a time: 64 for C = 10 and 37, 34 for C = 100; beyond it the kernel runs
    in chunks of samples."""
    return min(_lib.NLL_VEC_ROWS, _lib.NLL_VEC_SLAB // (C | 1))


@pytest.mark.parametrize("gain", [None, 24.0], ids=["ordinary", "x24"])
@pytest.mark.parametrize("C", [10, 37, 100])
def test_nll_vector_grad_equals_its_numpy_restatement(C, gain):
    """nll_vector_grad against nll_vector_numpy on the device's own logits, (T, B) in {(1, 1), (10, 7), (33, 5)} and a T on each side of the
    kernel's staging limit, ordinary and x24 logits: the value within 1e-9 relative (the figure
    tests/test_temperature.py::test_nll_grid_equals_its_numpy_restatement derives for <= 1e4 terms), the gradients within
    1e-9 * max(1, max |l|) (each of the <= 1e4 terms carries a factor |l|).  Accumulating two batches equals numpy on the concatenation to
    rtol 1e-12; two identical calls are torch.equal."""
    assert [_staging_limit(c) for c in (10, 37, 100)] == [64, 64, 34]
    lim = _staging_limit(C)
    m = _model(dict(EXIT_ONLY_10, out_dim=C), gain=gain)
    eng = m.engine(torch.device(DEV), max_batch=7, dtype="f16x2")
    full = eng.forward_samples(synthetic_images(7, seed=41).to(DEV), lim + 1, seed=17)
    E = full.shape[1]
    rng = np.random.default_rng(C)
    labels_all = rng.integers(0, C, 7)
    a = rng.uniform(0.4, 2.2, (E, C))
    b = rng.uniform(-1.0, 1.0, (E, C))
    lmax = float(full.abs().max())
    print(f"C {C} gain {gain}: max |logit| {lmax:.0f}, staging limit {lim}")
    for T, B in ((1, 1), (10, 7), (33, 5), (lim, 3), (lim + 1, 3)):
        logits = full[:T, :, :B].contiguous()
        y = torch.from_numpy(labels_all[:B])
        got = eng.nll_vector_grad(logits, y, a, b)
        again = eng.nll_vector_grad(logits, y, a, b)
        assert all(torch.equal(p, q) for p, q in zip(got, again))
        f, ga, gb = (t.cpu().numpy() for t in got)
        rf, rga, rgb = nll_vector_numpy(logits.cpu().numpy(), labels_all[:B], a, b)
        assert np.isfinite(f).all() and np.isfinite(ga).all() and np.isfinite(gb).all()
        e_f = float((np.abs(f - rf) / np.where(rf == 0, 1.0, np.abs(rf))).max())     # (x24, one image: both sides can be exactly 0)
        e_g = max(float(np.abs(ga - rga).max()), float(np.abs(gb - rgb).max()))
        print(f"  T {T} B {B}: value {e_f:.2e} relative, gradients {e_g:.2e} absolute (bound {1e-9 * max(1.0, lmax):.2e})")
        assert e_f <= 1e-9, (T, B, e_f)
        assert e_g <= 1e-9 * max(1.0, lmax), (T, B, e_g)
    # two batches accumulated into one triple = numpy on the concatenation
    p, q = full[:10, :, :3].contiguous(), full[:10, :, 3:7].contiguous()
    out = eng.nll_vector_grad(p, torch.from_numpy(labels_all[:3]), a, b)
    out = eng.nll_vector_grad(q, torch.from_numpy(labels_all[3:7]), a, b, out=out)
    ref = nll_vector_numpy(full[:10].cpu().numpy(), labels_all, a, b)
    for g_, r_ in zip(out, ref):
        np.testing.assert_allclose(g_.cpu().numpy(), r_, rtol=1e-12, atol=1e-12 * max(1.0, lmax))


# ---- 7. the fit, end to end -------------------------------------------------------------------------------------------------------
def test_vector_scaling_fit_end_to_end(tmp_path, monkeypatch):
    """VectorScaling over a three-batch loader of 8 images (T = 10, C = 100) with teacher labels drawn from a class-wise scaled softmax of the
    model's own mean logits: nll_after <= nll_start (the scalar fit's NLL) at every exit; nll_vector_numpy at the returned float32
    parameters on the logits copied to the host equals nll_after to rtol 1e-9; after apply() the model has no temperature and engines /
    FullAnalysis run under the scaling; save() round-trips; a refit after apply() gives the same result."""
    C, Bb, T, seed = 100, 8, 10, 5
    m = _model(EXIT_ONLY_100)
    m.engine_dtype = "f16x2"
    x = synthetic_images(3 * Bb, seed=31)
    eng = m.engine(torch.device(DEV), max_batch=Bb)
    raw = np.concatenate([eng.forward_samples(x[k * Bb:(k + 1) * Bb].to(DEV), T, seed=seed + k).cpu().numpy() for k in range(3)], axis=2)
    rng = np.random.default_rng(7)
    a_star, b_star = rng.uniform(0.5, 3.0, C), rng.uniform(-1.5, 1.5, C)
    z = raw.mean(0)[-1].astype(np.float64) * a_star + b_star                     # [N, C]
    p = np.exp(z - z.max(-1, keepdims=True))
    labels = np.array([rng.choice(C, p=q / q.sum()) for q in p])
    y = torch.from_numpy(labels)
    loader = [(x[k * Bb:(k + 1) * Bb], y[k * Bb:(k + 1) * Bb]) for k in range(3)]
    m.set_exit_temperature(2.0)                                                  # (apply() has something to clear)
    vs = VectorScaling(m, loader, gpu=0, mc_passes=T, seed=seed)
    r = vs.fit(max_iter=12)
    print(f"fit: nll {r['nll_start']} -> {r['nll_after']}, iterations {r['iterations']}, |g| {r['grad_norm']}, converged {r['converged']}")
    assert r["n"] == 3 * Bb and r["scale"].dtype == r["bias"].dtype == np.float32 and r["scale"].shape == r["bias"].shape == (4, C)
    assert (r["nll_after"] <= r["nll_start"]).all() and (r["nll_after"] < r["nll_start"]).any()
    host = nll_vector_numpy(raw, labels, r["scale"].astype(np.float64), r["bias"].astype(np.float64))[0]
    np.testing.assert_allclose(r["nll_after"], host, rtol=1e-9, atol=0)
    assert np.abs(r["bias"].astype(np.float64).sum(1)).max() <= 1e-4             # the zero-sum gauge (float32 rounding of 100 entries)
    scale, bias = vs.apply()
    assert m.exit_temperature is None and np.array_equal(scale, r["scale"]) and np.array_equal(bias, r["bias"])
    eng = m.engine(torch.device(DEV), max_batch=Bb)
    assert np.array_equal(eng.vector_scaling[0], r["scale"]) and eng.temperature == [1.0] * 4
    fa = FullAnalysis(m, loader, gpu=0, mc_dropout=True, mc_passes=T, seed=seed, macro_batches=1)
    want = np.concatenate([eng.predict(xb.to(DEV), T, seed=seed + k)["mean"].cpu().numpy() for k, (xb, _) in enumerate(loader)], axis=1)
    np.testing.assert_allclose(fa.preds, want, rtol=0, atol=1e-12)
    mean, _ = scale_logits(raw, r["scale"], r["bias"])
    assert float(np.abs(want - mean).max()) <= 1e-5
    monkeypatch.chdir(tmp_path)
    saved = np.load(vs.save("t"))
    assert np.array_equal(saved["scale"], r["scale"]) and np.array_equal(saved["bias"], r["bias"]) and np.array_equal(saved["nll_after"], r["nll_after"])
    r2 = VectorScaling(m, loader, gpu=0, mc_passes=T, seed=seed).fit(max_iter=12)        # raw logits do not depend on the scaling set
    assert np.array_equal(r2["scale"], r["scale"]) and np.array_equal(r2["bias"], r["bias"]) and np.array_equal(r2["nll_after"], r["nll_after"])


# ---- 8. ABI errors ----------------------------------------------------------------------------------------------------------------
def test_abi_errors_on_a_live_engine():
    m = _model(EXIT_ONLY_10)
    eng = MCDEngine(m, DEV, max_batch=4)
    E, C = eng.n_exits, eng.out_dim
    a, b = _coeffs(E, C)
    eng.set_temperature(2.0)
    with pytest.raises(ValueError):
        eng.set_vector_scaling(a, b)
    ad, bd = torch.from_numpy(a).to(DEV), torch.from_numpy(b).to(DEV)
    lib = eng.lib
    assert lib.bmi_engine_set_vector_scaling(eng.handle, ad.data_ptr(), bd.data_ptr(), E, C) == -22
    eng.set_temperature(None)
    assert lib.bmi_engine_set_vector_scaling(eng.handle, ad.data_ptr(), bd.data_ptr(), E + 1, C) == -22
    assert lib.bmi_engine_set_vector_scaling(eng.handle, ad.data_ptr(), bd.data_ptr(), E, C + 1) == -22
    eng.set_vector_scaling(a, b)
    with pytest.raises(ValueError):
        eng.set_temperature(2.0)
    import ctypes
    assert lib.bmi_engine_set_temperature(eng.handle, (ctypes.c_float * E)(*([2.0] * E)), E) == -22
    eng.set_temperature(1.0)                                                     # all ones is off: allowed
    # a scratch too small: BMI_ERR_NOMEM, nothing written
    T, B = 3, 4
    logits = eng.forward_samples(synthetic_images(B, seed=1).to(DEV), T, seed=0)
    y = torch.zeros(B, dtype=torch.int32, device=DEV)
    a64, b64 = ad.double(), bd.double()
    out = [torch.zeros(E, dtype=torch.float64, device=DEV), torch.zeros(E, C, dtype=torch.float64, device=DEV),
           torch.zeros(E, C, dtype=torch.float64, device=DEV)]
    need = int(lib.bmi_nll_vector_scratch_bytes(E, B, C))
    assert need == E * B * (2 * C + 1) * 8
    scratch = torch.zeros(need, dtype=torch.uint8, device=DEV)
    rc = lib.bmi_nll_vector_scaling_grad(logits.data_ptr(), T, E, B, C, y.data_ptr(), a64.data_ptr(), b64.data_ptr(), out[0].data_ptr(),
                                         out[1].data_ptr(), out[2].data_ptr(), scratch.data_ptr(), need - 1, None)
    torch.cuda.synchronize()
    assert rc == -12 and not any(bool(o.any()) for o in out) and not bool(scratch.any())
