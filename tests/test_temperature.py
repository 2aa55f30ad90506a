"""-m gpu: per-exit temperature scaling — the tempered fused exit head (bmi_engine_set_temperature) and the on-device NLL fit
(bmi_nll_temperature_grid).  Off is bit for bit the engine without a temperature; under a temperature the head's moments are those of the
tempered per-sample softmax of the SAME engine's raw logits, and track the reference-pinned golden logits within the softmax's Lipschitz
bound; chunking / t-range / image-share invariances, the entropy plane, early exit, adaptive sampling, graphs, FullAnalysis and the auto
engine choice compose with it; the fit kernel equals its numpy restatement and the loader-level fit equals the host search."""
import copy
import io

import numpy as np
import pytest
import torch

from bayesnn_fpga_amd.engine import BatchesInFlight, MCDEngine
from bayesnn_fpga_amd.models.resnet18.resnet18 import ResNet18MCEarlyExit
from bayesnn_fpga_amd.synthetic import synthetic_images, synthetic_weights_
from bayesnn_fpga_amd.train import confidence_exiting as cex
from bayesnn_fpga_amd.train.calibration import TemperatureScaling, nll_grid_numpy, temper_logits, zoom_search
from bayesnn_fpga_amd.train.metrics import ece_hist_binary
from bayesnn_fpga_amd.train.results_analyzer import FullAnalysis
from bayesnn_fpga_amd.train.uncertainty import decompose_logits, entropy_rows
from tests import test_adaptive_sampling as tas
from tests import test_staged_exit as tse
from tests.helpers import build_seeded
from tests.test_uncertainty import CONFIGS, DTYPES, _golden_model, _invariance_engines, _np, _sums

pytestmark = [pytest.mark.gpu, pytest.mark.usefixtures("fp16_engine_default")]
DEV = "cuda:0"
HEADS = ("ex1linear", "ex2linear", "ex3linear", "linear")
EXIT_ONLY_10 = dict(dropout_exit=True, dropout=None, dropout_p=0.25, out_dim=10)
EXIT_ONLY_100 = dict(dropout_exit=True, dropout=None, dropout_p=0.25, out_dim=100)
BLOCK_10 = dict(dropout_exit=True, dropout="block", dropout_p=0.25, out_dim=10)


def _taus(E):
    """uniform 0.5, uniform 2.5, distinct per exit (one of them exactly 1)."""
    return {"uniform_0.5": [0.5] * E, "uniform_2.5": [2.5] * E, "distinct": [0.7, 1.0, 1.9, 3.1, 0.45][:E]}


def _model(kw, gain=None):
    m = synthetic_weights_(build_seeded(ResNet18MCEarlyExit, kw), 0)
    if gain:                     # the "trained-like" twin of bench.py's tolerance leg: every classifier x 24
        with torch.no_grad():
            for n in HEADS:
                getattr(m, n).weight.mul_(gain)
    return m.to(DEV).eval()


# ---- 1. off is off ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("head_batch", [0, 1])
@pytest.mark.parametrize("dt", DTYPES)
def test_off_is_off(dt, head_batch):
    """tau = None, tau = ones and set-then-reset give S and H torch.equal to an engine that never heard of a temperature (T = 40: two
    sample groups, the join kernel too), on an exit-only model (the heads run as one pack when head_batch = 1) and one with a stochastic trunk."""
    for kw in (EXIT_ONLY_100, BLOCK_10):
        m = _model(kw)
        B, T, seed = 6, 40, 3
        x = synthetic_images(B, seed=5).to(DEV)
        ref = MCDEngine(m, DEV, max_batch=B, dtype=dt)
        ref.set_option("head_batch", head_batch)
        S0, H0 = ref.new_uncertainty_sums(B)
        ref.accumulate_uncertainty(x, S0, H0, 0, T, seed)
        S0m = ref.accumulate(x, ref.new_moments(B), 0, T, seed)
        eng = MCDEngine(m, DEV, max_batch=B, dtype=dt)
        eng.set_option("head_batch", head_batch)

        def run():
            S, H = eng.new_uncertainty_sums(B)
            eng.accumulate_uncertainty(x, S, H, 0, T, seed)
            return S, H, eng.accumulate(x, eng.new_moments(B), 0, T, seed)
        for tau in (None, [1.0] * eng.n_exits, 1.0):
            eng.set_temperature(tau)
            S, H, Sm = run()
            assert torch.equal(S, S0) and torch.equal(H, H0) and torch.equal(Sm, S0m), tau
        eng.set_temperature(2.0)
        assert eng.temperature == [2.0] * eng.n_exits
        S, H, Sm = run()
        assert not torch.equal(S[0], S0[0]) and not torch.equal(H, H0)
        assert torch.equal(S[2], S0[2]) and torch.equal(Sm[2], S0m[2])        # SL stays the raw logit sum
        eng.set_temperature(None)
        S, H, Sm = run()
        assert torch.equal(S, S0) and torch.equal(H, H0) and torch.equal(Sm, S0m)


# ---- 2. self-consistency ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("name", CONFIGS)
def test_self_consistency(name, dt):
    """mean / var against temper_logits of the SAME engine's forward_samples logits: 1e-5 for the mean — the figure tests/test_uncertainty.py
    grants the head's fp32 per-sample arithmetic — and 4e-5 for the variance (E[p^2] - mean^2 with p <= 1: four times the error in p);
    logit_mean and forward_samples are bit-equal to the run without a temperature."""
    m, g, x, T, seed = _golden_model(name)
    B = x.shape[0]
    eng = m.engine(x.device, max_batch=B, dtype=dt)
    off = eng.predict(x, T, seed=seed)
    logits_off = eng.forward_samples(x, T, seed=seed, cnt0=0)
    raw = logits_off.cpu().numpy()
    for tag, tau in _taus(eng.n_exits).items():
        eng.set_temperature(tau)
        r = eng.predict(x, T, seed=seed)
        eng.check_finite()
        mean, var = temper_logits(raw, tau)
        e_mean = float(np.abs(r["mean"].cpu().numpy() - mean).max())
        e_var = float(np.abs(r["var"].cpu().numpy() - var).max())
        print(f"{name} {dt} {tag}: |mean - tempered| {e_mean:.2e}, |var - tempered| {e_var:.2e}")
        assert e_mean <= 1e-5 and e_var <= 4e-5, (tag, e_mean, e_var)
        assert torch.equal(r["logit_mean"], off["logit_mean"])
        assert torch.equal(eng.forward_samples(x, T, seed=seed, cnt0=0), logits_off)
        assert not torch.equal(r["mean"], off["mean"])
    eng.set_temperature(None)


# ---- 3. against the reference-pinned logits ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", ["f16", "f16x2"])
@pytest.mark.parametrize("name", CONFIGS)
def test_against_the_reference_goldens(name, dt):
    """mean within d / (2 tau_min) + (d / tau_min)^2 + 1e-6 of temper_logits of the golden's per-pass logits, var within four times that,
    d = max |engine per-pass logits - golden logits| measured here.

    Why: the softmax Jacobian dp_c / dz_k = p_c (delta_ck - p_k) gives |dp_c| <= p_c (1 - p_c) |dz_c| + p_c sum_{k != c} p_k |dz_k|
    <= 2 p_c (1 - p_c) |dz|_inf <= |dz|_inf / 2, and dz = dl / tau: first order d / (2 tau_min) for every sample, hence for their mean;
    (d / tau_min)^2 covers the second-order remainder and 1e-6 the head's fp32 per-sample arithmetic.  The variance E[p^2] - mean^2 with
    p <= 1 moves by at most four times the error in p."""
    m, g, x, T, seed = _golden_model(name)
    B = x.shape[0]
    eng = m.engine(x.device, max_batch=B, dtype=dt)
    logits = eng.forward_samples(x, T, seed=seed, cnt0=0).cpu().numpy()
    ref_logits = g["logits"]
    assert logits.shape == ref_logits.shape
    d = float(np.abs(logits.astype(np.float64) - ref_logits).max())
    for tag, tau in _taus(eng.n_exits).items():
        tmin = min(tau)
        bound = d / (2 * tmin) + (d / tmin) ** 2 + 1e-6
        eng.set_temperature(tau)
        r = _np(eng.predict(x, T, seed=seed))
        eng.check_finite()
        mean, var = temper_logits(ref_logits, tau)
        e_mean, e_var = float(np.abs(r["mean"] - mean).max()), float(np.abs(r["var"] - var).max())
        print(f"{name} {dt} {tag}: d {d:.2e}, bound {bound:.2e}, |mean| {e_mean:.2e}, |var| {e_var:.2e}")
        assert e_mean <= bound, f"{tag} mean: {e_mean:.3e} > {bound:.3e} (d = {d:.3e})"
        assert e_var <= 4 * bound, f"{tag} var: {e_var:.3e} > {4 * bound:.3e} (d = {d:.3e})"
    eng.set_temperature(None)


@pytest.mark.parametrize("kw", [BLOCK_10, EXIT_ONLY_100], ids=["block", "exit_only_c100"])
def test_project_bar_against_the_oracle_at_tau_at_least_one(kw):
    """The project's bar directly: at tau >= 1 on the synthetic models mean and var are within 1e-3 of the tempering of the CPU oracle's
    passes (oracle.mcd.mcd_passes) — tempering with tau >= 1 contracts logit errors, so the bar of the untempered path carries over."""
    from oracle import mcd
    from oracle import resnet18 as oresnet
    m = _model(kw)
    ref_model = synthetic_weights_(build_seeded(oresnet.ResNet18MCEarlyExit, kw), 0)
    B, T, seed = 8, 6, 42
    x = synthetic_images(B, seed=1234)
    ref_logits, _ = mcd.mcd_passes(ref_model, x, T, seed)
    eng = m.engine(torch.device(DEV), max_batch=B)
    for tau in ([1.0, 1.5, 2.0, 4.0], [2.5] * 4):
        eng.set_temperature(tau)
        r = _np(eng.predict(x.to(DEV), T, seed=seed))
        mean, var = temper_logits(ref_logits, tau)
        e_mean, e_var = float(np.abs(r["mean"] - mean).max()), float(np.abs(r["var"] - var).max())
        print(f"tau {tau}: |mean - oracle| {e_mean:.2e}, |var - oracle| {e_var:.2e}")
        assert e_mean <= 1e-3 and e_var <= 1e-3


# ---- 4. invariances under a temperature -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kw", [EXIT_ONLY_100, BLOCK_10], ids=["exit_only_c100", "block"])
def test_invariances_under_temperature(kw):
    """tests/test_uncertainty.py's invariance assertions with a temperature set on the model (every engine built from it inherits it):
    70 samples in one call (three 32-sample groups joined in group order) against launches of at most 32 samples, T split in two t-ranges
    and image shares through image_offset — rtol 1e-12 on S and H; head_batch 1 against 0 bit for bit."""
    B, T, seed = 8, 70, 11
    model = _model(kw)
    model.set_exit_temperature([0.6, 1.0, 1.7, 2.5])
    x = synthetic_images(B, seed=77).to(DEV)
    e_def, e32 = _invariance_engines(model, B)
    assert e_def.temperature == pytest.approx([0.6, 1.0, 1.7, 2.5]) and e_def.chunk_samples >= T
    S, H = _sums(e_def, x, T, seed)
    runs = [_sums(e_def, x, T, seed, t_ranges=[(0, 32), (32, 32), (64, T - 64)]), _sums(e_def, x, T, seed, t_ranges=[(0, 29), (29, T - 29)]),
            _sums(e_def, x, T, seed, shares=[(0, 4), (4, 8)])]
    if kw["dropout"] is None:        # (with convs in the suffix two plans pick different fp16 conv kernels: tests/test_uncertainty.py)
        runs.append(_sums(e32, x, T, seed))
    for S2, H2 in runs:
        np.testing.assert_allclose(H2, H, rtol=1e-12, atol=0)
        np.testing.assert_allclose(S2, S, rtol=1e-12, atol=1e-12)
    e_def.set_temperature(None)
    S_off, _ = _sums(e_def, x, T, seed)
    assert not np.array_equal(S_off[0], S[0]) and np.array_equal(S_off[2], S[2])
    e_def.set_temperature(model.exit_temperature)
    e_def.set_option("head_batch", 0)
    S0, H0 = _sums(e_def, x, T, seed)
    assert np.array_equal(S0, S) and np.array_equal(H0, H)


# ---- 5. composition ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", ["f16", "f16x2"])
def test_predict_uncertainty_under_temperature(dt):
    """exp_entropy = the float64 mean entropy of the tempered per-sample softmax (the same engine's raw logits times inv, as fp32) to
    1e-5; pred_entropy = H(mean) to 1e-9."""
    m, g, x, T, seed = _golden_model("resnet18_mask8_exit_c100")
    eng = m.engine(x.device, max_batch=x.shape[0], dtype=dt)
    raw = eng.forward_samples(x, T, seed=seed, cnt0=0).cpu().numpy()
    for tau in _taus(eng.n_exits).values():
        eng.set_temperature(tau)
        r = _np(eng.predict_uncertainty(x, T, seed=seed, cnt0=0))
        inv = (1.0 / np.asarray(tau, np.float32).astype(np.float64)).astype(np.float32)
        dref = decompose_logits(raw * inv.reshape(1, -1, 1, 1))
        np.testing.assert_allclose(r["exp_entropy"], dref["exp_entropy"], rtol=0, atol=1e-5)
        np.testing.assert_allclose(r["pred_entropy"], entropy_rows(r["mean"]), rtol=0, atol=1e-9)
        np.testing.assert_allclose(r["mutual_info"], np.maximum(r["pred_entropy"] - r["exp_entropy"], 0), rtol=0, atol=1e-12)
    eng.set_temperature(None)


TAU_COMP = [0.6, 1.4, 2.2, 3.0]


@pytest.mark.parametrize("dt", ["f16", "f16x2"])
def test_predict_with_exit_under_temperature(dt):
    """tests/test_dynamic_exit.py's assertions with a temperature set: the exits are the reference's post-hoc rule on the full run UNDER
    THE SAME temperature, and every image's prediction at its exit equals that run's."""
    B, T, seed = 45, 6, 11
    m = _model(BLOCK_10)
    m.set_exit_temperature(TAU_COMP)
    eng = m.engine(torch.device(DEV), max_batch=B, dtype=dt)
    x = synthetic_images(B, seed=21).to(DEV)
    p_full = eng.predict(x, T, seed=seed)["mean"].cpu().numpy()
    conf = p_full.max(-1)
    for thr in (float(np.median(conf[1])), float(np.quantile(conf[2], 0.3))):
        want = cex.exit_layer(p_full.copy(), thr)
        r = eng.predict_with_exit(x, T, thr, seed=seed)
        got = r["exit_layer"].cpu().numpy()
        np.testing.assert_array_equal(got, want)
        if thr == float(np.median(conf[1])):          # about half of the images leave at exit 1, the others later
            assert len(set(got.tolist())) > 1
        np.testing.assert_allclose(r["best_preds"].cpu().numpy(), p_full[want, np.arange(B)], rtol=0, atol=1e-13)
        mean = r["mean"].cpu().numpy()
        for e in range(1, 4):
            gone = got < e
            assert np.all(mean[e][gone] == 0.0)
            np.testing.assert_allclose(mean[e][~gone], p_full[e][~gone], rtol=0, atol=1e-13)


@pytest.mark.parametrize("name", ["r18_exit_only", "r18_block_exit"])
def test_predict_early_exit_under_temperature(name):
    """tests/test_staged_exit.py's check with a temperature set: both rules, ensemble on and off — the decisions equal the numpy
    restatement on the full run's sums under the same temperature, computed rows are bit-equal to that run, the others stay zero."""
    B, T, seed = 45, 6, 11
    eng = tse._engine(name, "f16", B)
    eng.set_temperature(TAU_COMP)
    x = synthetic_images(B, seed=21).to(DEV)
    S_full, H_full = tse._full(eng, x, T, seed)
    for rule, ens in tse.RULES:
        stat = tse._stat(S_full[0], T, rule, ens)
        for thr in (float(np.quantile(stat[1], 0.25)), float(np.median(stat[1])), float(np.quantile(stat[1], 0.75))):
            got, act = tse._check_call(eng, x, T, seed, S_full, H_full, rule, ens, thr)
        assert len(set(got.tolist())) > 1, (rule, ens)


@pytest.mark.parametrize("name", ["r18_block", "r18_exit_only"])
def test_predict_adaptive_under_temperature(name):
    """tests/test_adaptive_sampling.py's check with a temperature set: both stop rules — every image's sums equal the fixed run's snapshot
    (same temperature) at its own t_used bit for bit, and t_used / converged equal the numpy re-derivation from those snapshots."""
    B, T_max, t_step, seed = 45, 12, 4, 11
    cls, kw = tas.MODELS[name]
    m = synthetic_weights_(build_seeded(cls, kw), 0).to(DEV).eval()
    m.set_exit_temperature(TAU_COMP)
    eng = m.engine(torch.device(DEV), max_batch=B, chunk_samples=t_step, dtype="f16")
    x = synthetic_images(B, seed=21).to(DEV)
    snap = tas.snapshots(eng, x, T_max, t_step, seed, with_H=True)
    e = eng.n_exits - 1
    for rule, q in (("sem", 0.4), ("margin", 0.6)):
        thr = tas.pick_threshold(snap, e, rule, q)
        S, H, t_used, conv, act = tas.run_adaptive(eng, x, T_max, t_step, thr, rule, seed, with_H=True)
        want_t, want_c, want_act = tas.rederive(snap, e, rule, thr, B)
        np.testing.assert_array_equal(t_used, want_t)
        np.testing.assert_array_equal(conv, want_c)
        assert act == want_act
        assert len(set(t_used.tolist())) > 1
        tas.check_truncation(eng, x, snap, S, H, t_used)


def test_tempering_keeps_images_in_the_net_on_the_trained_like_twin():
    """The x24 twin at confidence threshold 0.9: fewer images leave at exit 1 under tau = 4 than under tau = 1 (a cooler softmax is less
    confident).  Batch and seed chosen on the CPU oracle (oracle.mcd.mcd_passes of the same twin, B = 250, T = 6, seed 11, images seed 21):
    32 images pass 0.9 at exit 1 at tau = 1 and 28 at tau = 4, and no image's confidence is within 6e-3 of the threshold."""
    B, T, seed = 250, 6, 11
    m = _model(EXIT_ONLY_10, gain=24.0)
    eng = m.engine(torch.device(DEV), max_batch=B, dtype="f16x2")
    x = synthetic_images(B, seed=21).to(DEV)
    left = {}
    for tau in (1.0, 4.0):
        eng.set_temperature(tau)
        r = eng.predict_early_exit(x, T, 0.9, seed=seed, first_exit=1)
        left[tau] = int((r["exit_layer"].cpu().numpy() == 1).sum())
        conf1 = eng.predict(x, T, seed=seed)["mean"][1].cpu().numpy().max(-1)
        assert left[tau] == int((conf1 > 0.9).sum())
    print(f"images leaving at exit 1 at 0.9: tau 1 -> {left[1.0]}, tau 4 -> {left[4.0]}")
    assert left[4.0] < left[1.0]


def test_predict_graphed_after_set_temperature_equals_eager():
    B, T, seed = 8, 4, 9
    m = _model(EXIT_ONLY_10)
    x = synthetic_images(B, seed=12).to(DEV)
    pipe = BatchesInFlight(m, DEV, n=1, max_batch=B, dtype="f16")

    def graphed():
        """One graphed step, read after its stream has finished (the results are produced on pipe.last_stream)."""
        out = pipe.predict_graphed(x, T, seed)
        pipe.synchronize()
        return {k: v.clone() for k, v in out.items()}
    r0, r0b = graphed(), graphed()                                                     # the capture, then a replay of it
    assert all(torch.equal(r0[k], r0b[k]) for k in r0)
    pipe.set_temperature(2.0)
    assert not hasattr(pipe, "_graphs")
    for _ in range(2):                                                                 # capture, then replay
        r1 = graphed()
        eager = pipe.engines[0].predict(x, T, seed=seed)
        torch.cuda.synchronize()
        assert all(torch.equal(r1[k], eager[k]) for k in eager)
        assert not torch.equal(r1["mean"], r0["mean"]) and torch.equal(r1["logit_mean"], r0["logit_mean"])
    pipe.close()


def test_full_analysis_save_load_and_auto_follow_the_model_temperature(monkeypatch):
    B, T, seed = 4, 10, 7
    m = _model(BLOCK_10)
    x = synthetic_images(3 * B, seed=3)
    y = torch.arange(3 * B) % 10
    loader = [(x[i * B:(i + 1) * B], y[i * B:(i + 1) * B]) for i in range(3)]
    off = FullAnalysis(m, loader, gpu=0, mc_dropout=True, mc_passes=T, seed=seed, macro_batches=1).preds
    tau = [0.6, 1.4, 2.2, 3.0]
    m.set_exit_temperature(tau)
    assert m._engines == {} and m._fa_pipes == {}
    fa = FullAnalysis(m, loader, gpu=0, mc_dropout=True, mc_passes=T, seed=seed, macro_batches=1)
    eng = m.engine(torch.device(DEV), max_batch=B)
    assert eng.temperature == pytest.approx(tau)
    want = np.concatenate([eng.predict(xb.to(DEV), T, seed=seed + k)["mean"].cpu().numpy() for k, (xb, _) in enumerate(loader)], axis=1)
    np.testing.assert_allclose(fa.preds, want, rtol=0, atol=1e-12)
    assert np.abs(fa.preds - off).max() > 1e-3
    # torch.save / load round-trips the attribute, and the loaded model's engines run under it
    buf = io.BytesIO()
    torch.save(m, buf)
    buf.seek(0)
    m2 = torch.load(buf, weights_only=False)
    assert m2.exit_temperature == m.exit_temperature and type(m2.exit_temperature) is list
    r2 = m2.engine(torch.device(DEV), max_batch=B).predict(loader[0][0].to(DEV), T, seed=seed)["mean"].cpu().numpy()
    np.testing.assert_array_equal(r2, want[:, :B])
    assert copy.deepcopy(m).exit_temperature == m.exit_temperature
    # engine_dtype = "auto": the record is made again, under the new temperature
    m.engine_dtype = "auto"
    m.invalidate_engine()
    xc = loader[0][0].to(DEV)
    m.engine(torch.device(DEV), max_batch=B, calib=xc)
    rec1 = dict(m._auto[str(torch.device(DEV))])
    m.set_exit_temperature(None)
    assert m._auto == {}
    m.engine(torch.device(DEV), max_batch=B, calib=xc)
    rec2 = m._auto[str(torch.device(DEV))]
    assert rec2["dmean"] != rec1["dmean"]          # the fp16-vs-split comparison was made under another softmax


# ---- 6. the fit kernel ------------------------------------------------------------------------------------------------------------
def _device_logits(C, gain, B=250, T=100, seed=17):
    m = _model(EXIT_ONLY_100 if C == 100 else EXIT_ONLY_10, gain=gain)
    eng = m.engine(torch.device(DEV), max_batch=B, dtype="f16x2")
    x = synthetic_images(B, seed=41).to(DEV)
    return eng, eng.forward_samples(x, T, seed=seed)


@pytest.mark.parametrize("gain", [None, 24.0], ids=["ordinary", "x24"])
@pytest.mark.parametrize("C", [10, 100])
def test_nll_grid_equals_its_numpy_restatement(C, gain):
    """nll_grid against nll_grid_numpy on the device's own logits to 1e-9 relative, C in {10, 100} x T in {1, 10, 100} x B in {7, 250} x
    G in {1, 33}, tau down to 0.05, ordinary and x24 logits; everything finite.  (Each image's term carries a few ulp of float64 from
    exp / log; summing <= 1e4 of them stays below 1e-11; 1e-9 leaves two orders of margin for the device's libm.)  Accumulating two
    batches into one nll equals numpy on the concatenation to 1e-12; two identical calls give torch.equal results."""
    eng, full = _device_logits(C, gain)
    E = full.shape[1]
    rng = np.random.default_rng(C)
    labels_all = rng.integers(0, C, full.shape[2])
    print(f"C {C} gain {gain}: max |logit| {float(full.abs().max()):.0f}")
    worst = 0.0
    for T in (1, 10, 100):
        for B in (7, 250):
            logits = full[:T, :, :B].contiguous()
            y = torch.from_numpy(labels_all[:B])
            for G in (1, 33):
                tau = np.full((E, 1), 0.05, np.float32) if G == 1 else \
                    np.stack([np.exp(np.linspace(np.log(0.05), np.log(20.0), G)) * (1 + 0.01 * e) for e in range(E)]).astype(np.float32)
                got = eng.nll_grid(logits, y, tau)
                again = eng.nll_grid(logits, y, tau)
                assert torch.equal(got, again)
                got = got.cpu().numpy()
                ref = nll_grid_numpy(logits.cpu().numpy(), labels_all[:B], tau)
                assert np.isfinite(got).all() and np.isfinite(ref).all()
                err = float(np.abs(got / ref - 1).max())
                worst = max(worst, err)
                assert err <= 1e-9, (T, B, G, err)
    print(f"worst relative difference to numpy: {worst:.2e}")
    # two batches accumulated into one buffer = numpy on the concatenation
    a, b = full[:10, :, :100].contiguous(), full[:10, :, 100:250].contiguous()
    tau = np.stack([np.exp(np.linspace(np.log(0.05), np.log(20.0), 33))] * E).astype(np.float32)
    out = eng.nll_grid(a, torch.from_numpy(labels_all[:100]), tau)
    out = eng.nll_grid(b, torch.from_numpy(labels_all[100:250]), tau, out=out).cpu().numpy()
    ref = nll_grid_numpy(full[:10, :, :250].cpu().numpy(), labels_all[:250], tau)
    np.testing.assert_allclose(out, ref, rtol=1e-12, atol=0)


# ---- 7. the fit, end to end -------------------------------------------------------------------------------------------------------
FIT_SIZES = [1000, 1000, 1000, 600]       # four batches, the last one smaller
FIT_T, FIT_SEED = 10, 5


def _teacher_labels(logits, C, tau_star=3.0, seed=7):
    """Labels drawn from the final exit's predictive tempered at tau_star, fixed seed."""
    mean, _ = temper_logits(logits, tau_star)
    rng = np.random.default_rng(seed)
    return np.array([rng.choice(C, p=q / q.sum()) for q in mean[-1]])


def test_temperature_scaling_fit_end_to_end(tmp_path, monkeypatch):
    """TemperatureScaling.fit over a four-batch loader of the x24 twin (block + exit dropout, C = 10) with teacher labels drawn at tau* = 3 from the final exit:
    tau within 2 rtol of zoom_search run on the host over nll_grid_numpy of the same logits, identical at_bound, nll_after <= nll_before,
    the final exit's tau in a band around 3, hist-ECE of the final exit lower after apply(), ValueError over max_logit_bytes.

    The band comes from the CPU oracle (oracle.mcd.mcd_passes of the same twin, images, seeds and label draw, the host search over
    nll_grid_numpy; not from this code's output): there the final exit fits tau = 3.0788, the NLL's curvature at the optimum is 6.80,
    i.e. a standard error of 1 / sqrt(6.80) = 0.383 for the maximum-likelihood temperature at N = 3600; the band is 3 +- three standard
    errors.  The three early exits of the twin run to the upper end of the bracket on final-exit teacher labels (at_bound) in the oracle
    as well.  N = 3600 because the final exit's hist-ECE moves little (its prediction is dominated by the vote between samples, which a
    temperature barely changes): the oracle measures 0.0142 -> 0.0099 at N = 3600 and cannot resolve the sign at N = 900."""
    C, N = 10, sum(FIT_SIZES)
    m = _model(BLOCK_10, gain=24.0)
    m.engine_dtype = "f16x2"
    x = synthetic_images(N, seed=31)
    offs = np.concatenate([[0], np.cumsum(FIT_SIZES)])
    eng = m.engine(torch.device(DEV), max_batch=max(FIT_SIZES))
    raw = np.concatenate([eng.forward_samples(x[offs[k]:offs[k + 1]].to(DEV), FIT_T, seed=FIT_SEED + k).cpu().numpy()
                          for k in range(len(FIT_SIZES))], axis=2)
    labels = _teacher_labels(raw, C)
    y = torch.from_numpy(labels)
    loader = [(x[offs[k]:offs[k + 1]], y[offs[k]:offs[k + 1]]) for k in range(len(FIT_SIZES))]
    ts = TemperatureScaling(m, loader, gpu=0, mc_passes=FIT_T, seed=FIT_SEED)
    r = ts.fit(rtol=1e-4)
    host = zoom_search(lambda tau: nll_grid_numpy(raw, labels, tau), 4, rtol=1e-4)
    print(f"fit: tau {r['tau']}, host search {host['tau']}, nll {r['nll_before']} -> {r['nll_after']}, rounds {r['rounds']}")
    assert r["n"] == N
    np.testing.assert_allclose(r["tau"], host["tau"], rtol=2e-4, atol=0)
    np.testing.assert_array_equal(r["at_bound"], host["at_bound"])
    assert (r["nll_after"] <= r["nll_before"]).all()
    np.testing.assert_allclose(r["nll_before"], host["nll_before"], rtol=1e-9)
    assert abs(r["tau"][-1] - 3.0) <= FIT_BAND, r["tau"]
    onehot = np.eye(C)[labels]

    def final_exit_ece():
        fa = FullAnalysis(m, loader, gpu=0, mc_dropout=True, mc_passes=FIT_T, seed=FIT_SEED, macro_batches=1, ece="hist")
        return ece_hist_binary(fa.preds[-1], onehot)
    before = final_exit_ece()
    assert ts.apply() == pytest.approx([float(t) for t in r["tau"]])
    after = final_exit_ece()
    print(f"final exit hist-ECE: {before:.4f} -> {after:.4f}")
    assert after < before
    with pytest.raises(ValueError, match=str(N * FIT_T * 4 * C * 4)):
        TemperatureScaling(m, loader, gpu=0, mc_passes=FIT_T, seed=FIT_SEED, max_logit_bytes=N * FIT_T * 4 * C * 4 - 1).fit()
    monkeypatch.chdir(tmp_path)
    saved = np.load(ts.save("t"))
    np.testing.assert_array_equal(saved["tau"], r["tau"])


FIT_BAND = 3 * 0.383       # three standard errors of the oracle's fit (the docstring above)
