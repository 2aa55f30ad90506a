"""-m gpu: the uncertainty decomposition of the fused exit head (bmi_forward_mcd_entropy / bmi_finalize_uncertainty) — against the
engine's own per-sample logits on every engine type, against the reference's golden per-pass logits, invariance under chunking /
t-shards / image shares, degenerate nets, and UncertaintyAnalysis against FullAnalysis."""
import ctypes as C

import numpy as np
import pytest
import torch

from bayesnn_fpga_amd import _lib
from bayesnn_fpga_amd.engine import MCDEngine
from bayesnn_fpga_amd.models.extra import VGG11MC
from bayesnn_fpga_amd.models.resnet18.resnet18 import ResNet18EarlyExit, ResNet18MCEarlyExit
from bayesnn_fpga_amd.models.vgg19.vgg19 import VGG19MCEarlyExit
from bayesnn_fpga_amd.synthetic import synthetic_images, synthetic_labels, synthetic_weights_
from bayesnn_fpga_amd.train.results_analyzer import FullAnalysis
from bayesnn_fpga_amd.train.uncertainty import UncertaintyAnalysis, average_predictive_entropy, decompose_logits, entropy_rows
from tests.helpers import build_seeded, golden_kwargs, load_golden

pytestmark = [pytest.mark.gpu, pytest.mark.usefixtures("fp16_engine_default")]
DEV = "cuda:0"
DTYPES = ["f16", "bf16", "f32", "f16x2", "bf16x3"]
CONFIGS = ["resnet18_exit_only", "resnet18_block_exit", "resnet18_layer_exit", "resnet18_mask4_block_exit", "resnet18_mask8_exit_c100",
           "vgg19_exit_mc"]
QUANTITIES = ("pred_entropy", "exp_entropy", "mutual_info")


def _golden_model(name):
    g = load_golden(f"{name}.npz")
    cls = VGG19MCEarlyExit if name.startswith("vgg19") else ResNet18MCEarlyExit
    m = synthetic_weights_(build_seeded(cls, golden_kwargs(g)), 0).to(DEV).eval()
    x = synthetic_images(int(g["B"]), seed=1234).to(DEV)
    return m, g, x, int(g["T"]), int(g["seed"])


def _np(r):
    return {k: v.cpu().numpy() for k, v in r.items()}


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("name", CONFIGS)
def test_self_consistency_and_untouched_moments(name, dt):
    """exp_entropy = float64 mean entropy of the SAME engine's per-sample logits (forward_samples, same seed / cnt0) to 1e-5 — the device
    evaluates each sample's entropy in fp32 —, pred_entropy = H(mean) to 1e-9, and the moment sums are bit for bit accumulate()'s."""
    m, g, x, T, seed = _golden_model(name)
    B = x.shape[0]
    eng = m.engine(x.device, max_batch=B, dtype=dt)
    assert eng.dtype == dt
    S, H = eng.new_uncertainty_sums(B)
    eng.accumulate_uncertainty(x, S, H, 0, T, seed, 0)
    r = _np(eng.finalize_uncertainty(S, H, T))
    eng.check_finite()
    logits = eng.forward_samples(x, T, seed=seed, cnt0=0).cpu().numpy()
    d = decompose_logits(logits)
    np.testing.assert_allclose(r["exp_entropy"], d["exp_entropy"], rtol=0, atol=1e-5)
    np.testing.assert_allclose(r["pred_entropy"], entropy_rows(r["mean"]), rtol=0, atol=1e-9)
    np.testing.assert_allclose(r["mutual_info"], np.maximum(r["pred_entropy"] - r["exp_entropy"], 0), rtol=0, atol=1e-12)
    assert (r["mutual_info"] >= 0).all() and (r["pred_entropy"] <= np.log(logits.shape[-1]) + 1e-9).all()
    S0 = eng.accumulate(x, eng.new_moments(B), 0, T, seed, 0)
    assert torch.equal(S, S0)


@pytest.mark.parametrize("dt", ["f16", "f16x2"])
@pytest.mark.parametrize("name", CONFIGS)
def test_against_the_reference_goldens(name, dt):
    """Each quantity within 6 ln(C) d + d^2 (+ 1e-6 for the device's fp32 per-sample entropy) of the float64 decomposition of the golden's
    per-pass logits, d = max |engine per-pass logits - golden logits| measured here.

    Why that bound (first order in the logit perturbation, max-norm d).  For one sample, dH/dl_c = -p_c (log p_c + H), so
    |grad H|_1 <= sum_c p_c (-log p_c) + H = 2 H <= 2 ln C: the expected entropy, a mean of such terms, moves by at most 2 ln(C) d.  For
    H[p_mean], dH/dl_{t,c} = (p_{t,c} / T)(-log pm_c + sum_k p_{t,k} log pm_k) (the +1 terms cancel), whose 1-norm over (t, c) is at most
    (2 / T) sum_t CE(p_t, pm) = 2 H[pm] <= 2 ln C; 4 ln C is taken as margin.  Mutual information (a difference, clamped — 1-Lipschitz):
    the sum, 6 ln C.  d^2 covers the second-order remainder at the d of these engines (<= 2e-2)."""
    m, g, x, T, seed = _golden_model(name)
    B = x.shape[0]
    eng = m.engine(x.device, max_batch=B, dtype=dt)
    logits = eng.forward_samples(x, T, seed=seed, cnt0=0).cpu().numpy()
    ref_logits = g["logits"]
    assert logits.shape == ref_logits.shape
    d = float(np.abs(logits.astype(np.float64) - ref_logits).max())
    Cn = ref_logits.shape[-1]
    bound = 6 * np.log(Cn) * d + d * d + 1e-6
    ref = decompose_logits(ref_logits)
    r = _np(eng.predict_uncertainty(x, T, seed=seed, cnt0=0))
    eng.check_finite()
    for q in QUANTITIES:
        err = float(np.abs(r[q] - ref[q]).max())
        assert err <= bound, f"{q}: {err:.3e} > {bound:.3e} (d = {d:.3e})"


def _invariance_engines(model, B, dt="f16"):
    return MCDEngine(model, DEV, max_batch=B, dtype=dt), MCDEngine(model, DEV, max_batch=B, chunk_samples=32, dtype=dt)


def _sums(eng, x, T, seed, t_ranges=None, shares=None):
    B = x.shape[0]
    S, H = eng.new_uncertainty_sums(B)
    if shares:
        for lo, hi in shares:
            Sp, Hp = eng.new_uncertainty_sums(hi - lo)
            eng.accumulate_uncertainty(x[lo:hi], Sp, Hp, 0, T, seed, 0, image_offset=lo)
            S[:, :, lo:hi] += Sp
            H[:, lo:hi] += Hp
    else:
        for t0, n in (t_ranges or [(0, T)]):
            eng.accumulate_uncertainty(x, S, H, t0, n, seed, 0)
    return S.cpu().numpy(), H.cpu().numpy()


@pytest.mark.parametrize("kw", [dict(dropout_exit=True, dropout=None, dropout_p=0.25, out_dim=100),
                                dict(dropout_exit=True, dropout="block", dropout_p=0.25, out_dim=10),
                                dict(dropout_exit=True, dropout="block", dropout_p=0.25, out_dim=10, mask_type="mask", num_masks=4,
                                     mask_scale=4.0)], ids=["exit_only_c100", "block", "mask4"])
def test_invariance_chunks_tshards_image_shares_and_head_batch(kw):
    """H agrees with one call (70 samples: three 32-sample groups joined in group order) to rtol 1e-12 for launches of at most 32 samples
    (one group each: direct adds), T split into two t-ranges and image shares via image_offset; the batched-head launch (head_batch 1) and
    one launch per head (0) give bit-identical S and H.  An engine PLANNED for chunks of 32 against the default one: where the suffix is
    nothing but the heads (exit-only dropout); with convs in the suffix the planned batch x chunk picks the fp16 engine's conv kernels (DESIGN
    §4), so its per-sample logits — S as much as H — differ at fp16 rounding between two such engines (measured: S1 1.9e-5 relative), and
    the two plans are compared on the split engine (f16x2), whose kernels do not depend on the chunk."""
    B, T, seed = 8, 70, 11
    model = synthetic_weights_(build_seeded(ResNet18MCEarlyExit, kw), 0).to(DEV).eval()
    x = synthetic_images(B, seed=77).to(DEV)
    e_def, e32 = _invariance_engines(model, B)
    assert e_def.chunk_samples >= T
    S, H = _sums(e_def, x, T, seed)
    assert (H > 0).all()
    runs = [_sums(e_def, x, T, seed, t_ranges=[(0, 32), (32, 32), (64, T - 64)]), _sums(e_def, x, T, seed, t_ranges=[(0, 29), (29, T - 29)]),
            _sums(e_def, x, T, seed, shares=[(0, 4), (4, 8)])]
    if kw["dropout"] is None:
        runs.append(_sums(e32, x, T, seed))
    else:                         # the split engine's conv kernels do not depend on the planned chunk: the two plans agree there
        s_def, s32 = _invariance_engines(model, B, "f16x2")
        Ss, Hs = _sums(s_def, x, T, seed)
        S2s, H2s = _sums(s32, x, T, seed)
        np.testing.assert_allclose(H2s, Hs, rtol=1e-12, atol=0)
        np.testing.assert_allclose(S2s, Ss, rtol=1e-12, atol=1e-12)
    for S2, H2 in runs:
        np.testing.assert_allclose(H2, H, rtol=1e-12, atol=0)
        np.testing.assert_allclose(S2, S, rtol=1e-12, atol=1e-12)
    e_def.set_option("head_batch", 0)
    S0, H0 = _sums(e_def, x, T, seed)
    assert np.array_equal(S0, S) and np.array_equal(H0, H)
    St, Ht = _sums(e32, x, T, seed)
    e32.set_option("head_batch", 0)
    S1, H1 = _sums(e32, x, T, seed)
    assert np.array_equal(S1, St) and np.array_equal(H1, Ht)


def test_invariance_and_self_consistency_vgg11_dense_head():
    B, T, seed = 8, 40, 5
    model = synthetic_weights_(build_seeded(VGG11MC, dict(num_bayes_layer=3, dropout_p=0.25, out_dim=10)), 0).to(DEV).eval()
    x = synthetic_images(B, seed=78).to(DEV)
    e_def, e32 = _invariance_engines(model, B)
    S, H = _sums(e_def, x, T, seed)
    for S2, H2 in (_sums(e32, x, T, seed), _sums(e_def, x, T, seed, t_ranges=[(0, 17), (17, T - 17)])):
        np.testing.assert_allclose(H2, H, rtol=1e-12, atol=0)
        np.testing.assert_allclose(S2, S, rtol=1e-12, atol=1e-12)
    d = decompose_logits(e_def.forward_samples(x, T, seed=seed).cpu().numpy())
    np.testing.assert_allclose(H / T, d["exp_entropy"], rtol=0, atol=1e-5)
    r = _np(e_def.predict_uncertainty(x, T, seed=seed))
    assert (r["mutual_info"] > 1e-4).any()


def test_no_stochasticity_means_no_mutual_information():
    """ResNet18EarlyExit (no site) and p = 0: every sample is the same, MI <= 1e-6 (and >= 0: clamped)."""
    x = synthetic_images(6, seed=9).to(DEV)
    for cls, kw in ((ResNet18EarlyExit, dict(out_dim=10)), (ResNet18MCEarlyExit, dict(dropout_exit=True, dropout="block", dropout_p=0.0, out_dim=10))):
        model = synthetic_weights_(build_seeded(cls, kw), 0).to(DEV).eval()
        r = _np(model.engine(x.device, max_batch=6).predict_uncertainty(x, 40, seed=3))
        assert (r["mutual_info"] >= 0).all() and r["mutual_info"].max() <= 1e-6
        assert (r["pred_entropy"] > 0).all()


def test_peaky_c100_logits_give_no_nan():
    """C = 100 with the classifiers scaled until most probabilities underflow in fp32 (the log-softmax form never takes log 0): finite, and
    within test 2's bound (d = 0 here: the engine's own logits, float64 on the host) of the float64 decomposition."""
    kw = dict(dropout_exit=True, dropout=None, dropout_p=0.25, out_dim=100)
    model = synthetic_weights_(build_seeded(ResNet18MCEarlyExit, kw), 0)
    with torch.no_grad():
        for lin in (model.ex1linear, model.ex2linear, model.ex3linear, model.linear):
            lin.weight.mul_(300.0)
            lin.bias.mul_(300.0)
    model = model.to(DEV).eval()
    B, T, seed = 6, 12, 21
    x = synthetic_images(B, seed=10).to(DEV)
    eng = model.engine(x.device, max_batch=B, dtype="f16x2")
    logits = eng.forward_samples(x, T, seed=seed).cpu().numpy()
    spread = logits.max(-1, keepdims=True) - logits
    assert (spread > 104).any(), "the scaled logits must underflow some fp32 probabilities"
    r = _np(eng.predict_uncertainty(x, T, seed=seed))
    eng.check_finite()
    assert all(np.isfinite(r[q]).all() for q in QUANTITIES)
    ref = decompose_logits(logits)
    for q in QUANTITIES:
        np.testing.assert_allclose(r[q], ref[q], rtol=0, atol=1e-5)


def test_finalize_uncertainty_counts_a_nan_input():
    lib = _lib.lib()
    E, B, Cn, T = 2, 3, 10, 4
    g = torch.Generator().manual_seed(0)
    P = torch.rand(E, B, Cn, T, generator=g, dtype=torch.float64)
    P = P / P.sum(2, keepdim=True)
    S1 = P.sum(-1).contiguous()
    SH = torch.from_numpy(entropy_rows(P.permute(3, 0, 1, 2).numpy()).sum(0)).contiguous()
    S1[1, 2, 5] = float("nan")
    S1d, SHd = S1.to(DEV), SH.to(DEV)
    out = torch.empty(3, E, B, dtype=torch.float64, device=DEV)
    cnt = torch.zeros(1, dtype=torch.int32, device=DEV)
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    rc = lib.bmi_finalize_uncertainty(E, B, Cn, T, S1d.data_ptr(), SHd.data_ptr(), out[0].data_ptr(), out[1].data_ptr(), out[2].data_ptr(),
                                      cnt.data_ptr(), st)
    assert rc == _lib.BMI_OK
    o = out.cpu().numpy()
    assert int(cnt.item()) == 1
    assert np.isnan(o[0, 1, 2]) and np.isnan(o[2, 1, 2])
    ok = np.ones((E, B), bool)
    ok[1, 2] = False
    m = (S1 / T).numpy()
    np.testing.assert_allclose(o[0][ok], entropy_rows(m)[ok], rtol=0, atol=1e-12)
    np.testing.assert_allclose(o[1], SH.numpy() / T, rtol=0, atol=1e-15)
    np.testing.assert_allclose(o[2][ok], np.maximum(o[0] - o[1], 0)[ok], rtol=0, atol=1e-15)


@pytest.mark.parametrize("kw", [dict(dropout_exit=True, dropout="block", dropout_p=0.25, out_dim=10),
                                dict(dropout_exit=True, dropout="block", dropout_p=0.25, out_dim=10, mask_type="mask", num_masks=4,
                                     mask_scale=4.0)], ids=["mc", "mask4"])
def test_uncertainty_analysis_matches_full_analysis(kw, tmp_path, monkeypatch):
    """Over a 3-batch seeded loader: mean = FullAnalysis(...).preds (same seed, macro_batches = 1) to 1e-12, aPE = the reference's formula
    on those preds, the Masksembles counters end where FullAnalysis leaves them, and save() writes the arrays."""
    m = synthetic_weights_(build_seeded(ResNet18MCEarlyExit, kw), 0).to(DEV).eval()
    B, T, seed = 4, 10, 7
    x, y = synthetic_images(3 * B, seed=3), synthetic_labels(3 * B, 10, seed=4)
    loader = [(x[i * B:(i + 1) * B], y[i * B:(i + 1) * B]) for i in range(3)]
    ml = m.mask_layers()
    cnt_start = [l.cnt for l in ml]
    fa = FullAnalysis(m, loader, gpu=0, mc_dropout=True, mc_passes=T, seed=seed, macro_batches=1)
    cnt_fa = [l.cnt for l in ml]
    for l, c in zip(ml, cnt_start):
        l.cnt = c
    ua = UncertaintyAnalysis(m, loader, gpu=0, mc_passes=T, seed=seed)
    assert [l.cnt for l in ml] == cnt_fa
    if ml:
        assert cnt_fa[0] == (cnt_start[0] + 3 * T) % ml[0].n
    np.testing.assert_allclose(ua.mean, fa.preds, rtol=0, atol=1e-12)
    E = ua.mean.shape[0]
    for e in range(E):
        assert abs(ua.ape[e] - average_predictive_entropy(fa.preds[e])) <= 1e-12
    assert ua.mutual_info.shape == (E, 3 * B) and (ua.mutual_info >= 0).all() and (ua.mutual_info > 0).any()
    np.testing.assert_allclose(ua.mean_mi, ua.mutual_info.mean(1), rtol=0, atol=0)
    np.testing.assert_allclose(ua.ensemble_pred_entropy[0], ua.pred_entropy[0], rtol=0, atol=1e-9)
    assert len(ua.summary()) == E and np.array_equal(ua.labels, y.numpy())
    monkeypatch.chdir(tmp_path)
    f = np.load(ua.save("t"))
    np.testing.assert_array_equal(f["mutual_info"], ua.mutual_info)
