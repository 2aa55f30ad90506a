"""-m gpu: weighted exit ensembles on the device (csrc/ensemble.hip's WEIGHTED instantiations, the weighted staged exit rule;
bmi_engine_set_ensemble_weights / bmi_ensemble_moments_weighted) — the stand-alone entry against the host restatement, its two bit-for-bit
identities (uniform power-of-two rows = the unweighted kernel, one-hot rows = the single-exit slice), invariance under the split of T,
the engine's read-out on every golden config, the adaptive and the staged decisions against float64 re-derivations, and the bits of an
engine whose weights were set and taken away again (eager and as a captured graph)."""
import numpy as np
import pytest
import torch

from bayesnn_fpga_amd.engine import check_ensemble_weights
from bayesnn_fpga_amd.synthetic import synthetic_images, synthetic_labels
from bayesnn_fpga_amd.train.calibration import EnsembleWeights, mixture_weights_em
from bayesnn_fpga_amd.train.uncertainty import (UncertaintyAnalysis, average_predictive_entropy, decompose_ensemble_logits,
                                                weighted_exit_ensembles)
from tests.test_adaptive_sampling import pick_threshold, rederive
from tests.test_exit_ensemble import CONFIGS, _any_engine, _check_against_host, _golden_model, _np
from tests.test_staged_exit import _decide
from tests.test_staged_exit_ensemble import midpoint_near_median

pytestmark = [pytest.mark.gpu, pytest.mark.usefixtures("fp16_engine_default")]
DEV = "cuda:0"
ENS_KEYS = ("ens_mean", "ens_var", "ens_pred_entropy", "ens_exp_entropy", "ens_mutual_info")
SHAPES = [(19, 4, 3, 100), (100, 4, 3, 10), (7, 5, 2, 128), (5, 1, 2, 1), (9, 3, 2, 33)]      # (T, E, B, C)


def simplex_rows(E, seed, zeros=False):
    """Random rows on the simplex (row e: e + 1 entries); ``zeros``: every row of two or more entries holds one exact zero."""
    rng = np.random.default_rng(seed)
    W = np.zeros((E, E))
    for e in range(E):
        w = rng.random(e + 1) + 0.05
        if zeros and e >= 1:
            w[rng.integers(0, e + 1)] = 0.0
        W[e, :e + 1] = w / w.sum()
    return check_ensemble_weights(W, E)


def synthetic_logits(shape, scale=3.0):
    T, E, B, Cn = shape
    g = torch.Generator().manual_seed(T * 1000 + Cn)
    return (torch.randn(T, E, B, Cn, generator=g) * scale).to(DEV)


@pytest.mark.parametrize("zeros", [False, True], ids=["simplex", "with_zeros"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_stand_alone_entry_against_the_host_restatement(shape, zeros):
    T, E, B, Cn = shape
    eng = _any_engine()
    logits = synthetic_logits(shape)
    W = simplex_rows(E, seed=T + Cn, zeros=zeros)
    r = eng.ensemble_moments(logits, weights=W)
    eng.check_finite()
    _check_against_host(_np(r), decompose_ensemble_logits(logits.cpu().numpy(), weights=W), f"{shape} weighted")
    again = eng.ensemble_moments(logits, weights=W)
    assert all(torch.equal(r[k], again[k]) for k in r)
    # two calls on the halves of T leave the bits of one call
    h = T // 2
    first = eng.ensemble_moments(logits[:h].contiguous(), weights=W)
    both = eng.ensemble_moments(logits[h:].contiguous(), out=(first["Q"], first["QH"]), t_before=h, weights=W)
    assert all(torch.equal(r[k], both[k]) for k in r)
    tau = [0.5 + 0.7 * e for e in range(E)]
    rt = _np(eng.ensemble_moments(logits, tau=tau, weights=W))
    _check_against_host(rt, decompose_ensemble_logits(logits.cpu().numpy(), tau, weights=W), f"{shape} weighted, tempered")
    if E > 1:
        plain = eng.ensemble_moments(logits)
        assert (plain["ens_mean"] - r["ens_mean"]).abs().max().item() > 1e-4, "the weights must act"
        assert torch.equal(plain["Q"][:, 0], r["Q"][:, 0]) and torch.equal(plain["QH"][0], r["QH"][0])      # row 0 is exit 0 either way


@pytest.mark.parametrize("shape", [(19, 4, 3, 100), (7, 5, 2, 128)], ids=lambda s: "x".join(map(str, s)))
def test_uniform_power_of_two_rows_are_the_unweighted_kernels_bits(shape):
    """W[e][i] = 1 / (e + 1): where e + 1 is a power of two the products are exact scalings, which commute with rounding — rows 0, 1 and 3
    of Q1 / Q2 / QH are bmi_ensemble_moments' bit for bit.  Row 2 (1/3 is rounded, and every product with it) stays within T * 4 * 2^-53
    on Q1: three rounded products and the additions of three terms, each within 2^-53 of a value <= 1, per sample."""
    T, E = shape[:2]
    eng = _any_engine()
    logits = synthetic_logits(shape)
    plain, uni = eng.ensemble_moments(logits), eng.ensemble_moments(logits, weights=np.ones(E))
    for e in (0, 1, 3):
        assert torch.equal(plain["Q"][:, e], uni["Q"][:, e]) and torch.equal(plain["QH"][e], uni["QH"][e]), e
        for k in ENS_KEYS:
            assert torch.equal(plain[k][e], uni[k][e]), (k, e)
    err = (plain["Q"][0, 2] - uni["Q"][0, 2]).abs().max().item()
    print(f"{shape}: row 2, Q1: {err:.3e}")
    assert err <= T * 4 * 2.0 ** -53


def test_one_hot_rows_are_the_single_exit_slice_bit_for_bit():
    shape = (19, 4, 3, 100)
    E = shape[1]
    eng = _any_engine()
    logits = synthetic_logits(shape)
    single = [eng.ensemble_moments(logits[:, k:k + 1].contiguous()) for k in range(E)]
    for ks in ([0, 1, 2, 3], [0, 0, 0, 0], [0, 1, 0, 2], [0, 0, 2, 1]):
        W = np.zeros((E, E))
        for e, k in enumerate(ks):
            W[e, k] = 1.0
        r = eng.ensemble_moments(logits, weights=W)
        for e, k in enumerate(ks):
            assert torch.equal(r["Q"][:, e], single[k]["Q"][:, 0]) and torch.equal(r["QH"][e], single[k]["QH"][0]), (ks, e)
            for n in ENS_KEYS:
                assert torch.equal(r[n][e], single[k][n][0]), (ks, e, n)


@pytest.mark.parametrize("dt", ["f16", "f16x2"])
@pytest.mark.parametrize("name", CONFIGS)
def test_predict_ensemble_with_weights_on_the_golden_configs(name, dt):
    """predict_ensemble under weights against the host restatement on the SAME engine's per-sample logits, plain and tempered; S and H
    keep the bits of the run without weights; taking the weights away gives the first run's bits back."""
    m, g, x, T, seed = _golden_model(name)
    B = x.shape[0]
    eng = m.engine(x.device, max_batch=B, dtype=dt)
    E = eng.n_exits
    assert eng.ensemble_weights is None
    plain_sums = eng.accumulate_ensemble(x, *eng.new_ensemble_sums(B), 0, T, seed, 0)
    plain = eng.predict_ensemble(x, T, seed=seed, cnt0=0)
    logits = eng.forward_samples(x, T, seed=seed, cnt0=0).cpu().numpy()
    W = simplex_rows(E, seed=len(name), zeros=dt == "f16x2")
    tau = [0.6 + 0.45 * e for e in range(E)]
    eng.set_ensemble_weights(W)
    try:
        assert np.array_equal(eng.ensemble_weights, W)
        S, H, Q, QH = eng.accumulate_ensemble(x, *eng.new_ensemble_sums(B), 0, T, seed, 0)
        assert torch.equal(S, plain_sums[0]) and torch.equal(H, plain_sums[1])
        assert torch.equal(Q[:, 0], plain_sums[2][:, 0]) and not torch.equal(Q[:, 1:], plain_sums[2][:, 1:])
        r = _np(eng.finalize_ensemble(S, H, Q, QH, T))
        eng.check_finite()
        _check_against_host(r, decompose_ensemble_logits(logits, weights=W), f"{name}/{dt} weighted")
        assert all(np.array_equal(r[k], v) for k, v in _np(eng.predict_ensemble(x, T, seed=seed, cnt0=0)).items())
        np.testing.assert_allclose(r["ens_mean"], weighted_exit_ensembles(r["mean"], W), rtol=0, atol=1e-6)      # (the head's softmax is fp32)
        eng.set_temperature(tau)
        rt = _np(eng.predict_ensemble(x, T, seed=seed, cnt0=0))
        eng.check_finite()
        _check_against_host(rt, decompose_ensemble_logits(logits, tau, weights=W), f"{name}/{dt} weighted, tempered")
    finally:
        eng.set_temperature(None)
        eng.set_ensemble_weights(None)
    back = eng.predict_ensemble(x, T, seed=seed, cnt0=0)
    assert set(back) == set(plain) and all(torch.equal(back[k], plain[k]) for k in plain)


T_MAX, T_STEP = 12, 4


@pytest.mark.parametrize("name", ["resnet18_block_exit", "resnet18_mask8_exit_c100", "vgg19_exit_mc"])
def test_adaptive_stop_on_ensemble_under_weights(name):
    """accumulate_adaptive(ensemble=True, stop_on="ensemble") with weights: every image's S / H / Q / QH are the fixed WEIGHTED run's,
    done step by step, at its own t_used bit for bit, and t_used / converged / active_after_step equal the float64 numpy re-derivation of
    the stop rule from the weighted Q1 / Q2 snapshots."""
    m, g, x, _, seed = _golden_model(name)
    B = x.shape[0]
    eng = m.engine(x.device, max_batch=B, dtype="f16")
    E = eng.n_exits
    W = simplex_rows(E, seed=7, zeros=name.startswith("vgg"))
    unweighted = eng.accumulate_ensemble(x, *eng.new_ensemble_sums(B), 0, T_STEP, seed, 0)[2].cpu().numpy()
    eng.set_ensemble_weights(W)
    try:
        sums, snap = eng.new_ensemble_sums(B), {}
        for t0 in range(0, T_MAX, T_STEP):
            eng.accumulate_ensemble(x, *sums, t0, T_STEP, seed, 0)
            snap[t0 + T_STEP] = tuple(a.cpu().numpy().copy() for a in sums)
        assert not np.array_equal(snap[T_STEP][2][:, 1:], unweighted[:, 1:])
        qs = {t: (v[2],) for t, v in snap.items()}
        for rule, q, e in (("sem", 0.4, E - 1), ("margin", 0.6, E - 1), ("sem", 0.5, 1)):
            thr = pick_threshold(qs, e, rule, q)
            S, H, Q, QH = got = eng.new_ensemble_sums(B)
            t_used, conv, act = eng.accumulate_adaptive(x, S, T_MAX, thr, rule, T_STEP, e, seed, 0, H, 0, ensemble=True, stop_on="ensemble", Q=Q,
                                                        QH=QH)
            t_used, conv = t_used.cpu().numpy(), conv.cpu().numpy().astype(bool)
            want_t, want_c, want_act = rederive(qs, e, rule, thr, B)
            print(f"{name}/{rule}/exit {e}: threshold {thr:.6g}, t_used {t_used.tolist()}, active after steps {act}")
            np.testing.assert_array_equal(t_used, want_t)
            np.testing.assert_array_equal(conv, want_c)
            assert act == want_act
            got = [a.cpu().numpy() for a in got]
            for b in range(B):
                ref = snap[int(t_used[b])]
                for i in range(4):
                    a, r = (got[i][:, :, b], ref[i][:, :, b]) if got[i].ndim == 4 else (got[i][:, b], ref[i][:, b])
                    np.testing.assert_array_equal(a, r, err_msg=f"{rule}: sums {i} of image {b} at t_used={int(t_used[b])}")
        r = eng.predict_adaptive(x, T_MAX, -1.0, t_step=T_STEP, seed=seed, ensemble=True, stop_on="ensemble")
        # nobody retires: the sums of the fixed weighted run done in the same steps, and their read-out
        assert (r["t_used"] == T_MAX).all() and not r["converged"].any()
        assert np.array_equal(r["Q"].cpu().numpy(), snap[T_MAX][2]) and np.array_equal(r["QH"].cpu().numpy(), snap[T_MAX][3])
        ref = eng._finalize_ensemble_sums(r["Q"], r["QH"], T_MAX)
        assert all(torch.equal(r[k], ref[k]) for k in ref)
        eng.check_finite()
    finally:
        eng.set_ensemble_weights(None)


def _weighted_stat(S1, T, W, rule):
    """float64 [E, B]: the weighted rule's statistic in the kernel's order — p = sum_{i<=e} W[e][i] * (S1[i] / T), from 0.0 in exit order."""
    p = weighted_exit_ensembles(S1 / T, W)
    top = -np.sort(-p, axis=2)
    return top[:, :, 0] - top[:, :, 1] if rule == "margin" else top[:, :, 0]


@pytest.mark.parametrize("first_exit", [0, 1])
@pytest.mark.parametrize("name", ["resnet18_exit_only", "resnet18_block_exit"])
def test_staged_exit_rule_and_readout_under_weights(name, first_exit):
    """accumulate_early_exit(ensemble=True) with Q / QH and weights: exit_layer equals the float64 host re-derivation of the WEIGHTED rule
    from the full run's means; the rows of the exits an image reached are the full weighted run's bit for bit, the others stay zero."""
    m, g, x, T, seed = _golden_model(name)
    B = x.shape[0]
    eng = m.engine(x.device, max_batch=B, dtype="f16")
    E = eng.n_exits
    W = simplex_rows(E, seed=3 + first_exit, zeros=first_exit == 1)
    eng.set_ensemble_weights(W)
    try:
        full = [a.cpu().numpy() for a in eng.accumulate_ensemble(x, *eng.new_ensemble_sums(B), 0, T, seed, 0)]
        for rule in ("confidence", "margin"):
            stat = _weighted_stat(full[0][0], T, W, rule)
            thr = midpoint_near_median(stat[first_exit])
            want = _decide(stat, thr, first_exit)
            S, H, Q, QH = eng.new_ensemble_sums(B)
            xl, act = eng.accumulate_early_exit(x, S, T, thr, seed=seed, first_exit=first_exit, rule=rule, ensemble=True, H=H, Q=Q, QH=QH)
            xl = xl.cpu().numpy()
            print(f"{name}/first_exit={first_exit}/{rule}: threshold {thr:.6g}, exits {xl.tolist()}, active after {act}")
            np.testing.assert_array_equal(xl, want)
            Qn, QHn = Q.cpu().numpy(), QH.cpu().numpy()
            for e in range(E):
                reached = xl >= e
                np.testing.assert_array_equal(Qn[:, e][:, reached], full[2][:, e][:, reached], err_msg=f"Q rows of exit {e}")
                np.testing.assert_array_equal(QHn[e][reached], full[3][e][reached], err_msg=f"QH rows of exit {e}")
                np.testing.assert_array_equal(S.cpu().numpy()[:, e][:, reached], full[0][:, e][:, reached], err_msg=f"S rows of exit {e}")
                assert not Qn[:, e][:, ~reached].any() and not QHn[e][~reached].any()
            r = eng.predict_early_exit(x, T, thr, seed=seed, first_exit=first_exit, rule=rule, ensemble=True, ensemble_readout=True)
            assert np.array_equal(r["exit_layer"].cpu().numpy(), want)
            best = weighted_exit_ensembles(r["mean"].cpu().numpy(), W)[want, np.arange(B)]
            np.testing.assert_allclose(r["best_preds"].cpu().numpy(), best, rtol=0, atol=1e-15)
            np.testing.assert_allclose(r["best_ens"]["mean"].cpu().numpy(), best, rtol=0, atol=1e-6)
        eng.check_finite()
    finally:
        eng.set_ensemble_weights(None)


def test_set_then_none_round_trip_keeps_the_parents_bits_eager_and_captured():
    """Weights set on the model reach every engine built from it; taken away again — on the model (engines rebuilt) or on an engine —
    predict_ensemble, the adaptive and the staged entry return the bits of a model that never had weights, also as a hipGraph captured
    after the round trip; a graph captured UNDER weights replays the eager weighted bits."""
    m, g, x, T, seed = _golden_model("resnet18_block_exit")
    B = x.shape[0]
    dev = torch.device(DEV)

    def run_all(eng):
        out = dict(eng.predict_ensemble(x, T, seed=seed))
        a = eng.predict_adaptive(x, 8, 0.05, t_step=4, seed=seed, ensemble=True, stop_on="ensemble")
        s = eng.predict_early_exit(x, T, 0.3, seed=seed, ensemble=True, ensemble_readout=True)
        out.update({"adaptive_" + k: v for k, v in a.items() if isinstance(v, torch.Tensor)})
        out.update({"staged_" + k: v for k, v in s.items() if isinstance(v, torch.Tensor)})
        return {k: v.clone() for k, v in out.items()}

    parent = run_all(m.engine(dev, max_batch=B, dtype="f16"))
    W = simplex_rows(4, seed=1)
    m.set_exit_ensemble_weights(W)
    eng = m.engine(dev, max_batch=B, dtype="f16")
    assert np.array_equal(eng.ensemble_weights, W)
    weighted = run_all(eng)
    assert not torch.equal(weighted["ens_mean"], parent["ens_mean"]) and torch.equal(weighted["mean"], parent["mean"])
    _check_against_host(_np({k: weighted[k] for k in ENS_KEYS}),
                        decompose_ensemble_logits(eng.forward_samples(x, T, seed=seed).cpu().numpy(), weights=W), "model-level weights")

    def capture(eng):
        xs = x.clone()
        S, H, Q, QH = eng.new_ensemble_sums(B)
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            eng.accumulate_ensemble(xs, S, H, Q, QH, 0, T, seed)
        torch.cuda.current_stream().wait_stream(side)
        graph, out = torch.cuda.CUDAGraph(), {}
        with torch.cuda.graph(graph):
            S._base.zero_()
            eng.accumulate_ensemble(xs, S, H, Q, QH, 0, T, seed)
            out.update(eng.finalize_ensemble(S, H, Q, QH, T))
        return graph, out, (S, xs)

    graph_w, out_w, keep_w = capture(eng)
    graph_w.replay()
    torch.cuda.synchronize()
    assert all(torch.equal(out_w[k], weighted[k]) for k in out_w)
    eng.set_ensemble_weights(None)                                   # on the engine
    assert eng.ensemble_weights is None
    back = run_all(eng)
    assert set(back) == set(parent) and all(torch.equal(back[k], parent[k]) for k in parent)
    graph, out, keep = capture(eng)
    graph.replay()
    torch.cuda.synchronize()
    assert all(torch.equal(out[k], parent[k]) for k in out)
    graph_w.replay()                                                 # the earlier capture keeps the weights it was captured with
    torch.cuda.synchronize()
    assert all(torch.equal(out_w[k], weighted[k]) for k in out_w)
    m.set_exit_ensemble_weights(None)                                # on the model: engines dropped and rebuilt
    eng2 = m.engine(dev, max_batch=B, dtype="f16")
    assert eng2 is not eng and eng2.ensemble_weights is None
    again = run_all(eng2)
    assert all(torch.equal(again[k], parent[k]) for k in parent)


def test_uncertainty_analysis_and_the_fit_follow_the_models_weights():
    """UncertaintyAnalysis(ensemble=True) on a model with weights holds the per-batch weighted predict_ensemble results; EnsembleWeights'
    table is mean[e, n, y_n] of predict under the walk's seeds and its rows are mixture_weights_em's."""
    m, g, x4, T, seed = _golden_model("resnet18_block_exit")
    B = x4.shape[0]
    x, y = synthetic_images(2 * B, seed=3), synthetic_labels(2 * B, 10, seed=4)
    loader = [(x[i * B:(i + 1) * B], y[i * B:(i + 1) * B]) for i in range(2)]
    m.engine_dtype = "f16"
    ew = EnsembleWeights(m, loader, gpu=0, mc_passes=T, seed=seed)
    r = ew.fit()
    eng = m.engine(torch.device(DEV), max_batch=B)
    A = np.concatenate([eng.predict(bx.to(DEV), T, seed + k)["mean"].cpu().numpy()[:, np.arange(B), np.asarray(by)]
                        for k, (bx, by) in enumerate(loader)], axis=1)
    assert np.array_equal(ew.table, A)
    for e in range(4):
        assert np.array_equal(r["weights"][e, :e + 1], mixture_weights_em(A[:e + 1])["w"]) and r["nll_after"][e] <= r["nll_uniform"][e]
    W = ew.apply()
    assert np.array_equal(m.exit_ensemble_weights, r["weights"]) and np.array_equal(W, r["weights"])
    ua = UncertaintyAnalysis(m, loader, gpu=0, mc_passes=T, seed=seed, ensemble=True)
    eng = m.engine(torch.device(DEV), max_batch=B)
    assert np.array_equal(eng.ensemble_weights, W)
    for k, (bx, _) in enumerate(loader):
        p = _np(eng.predict_ensemble(bx.to(DEV), T, seed + k))
        sl = slice(k * B, (k + 1) * B)
        assert np.array_equal(ua.ensemble_var[:, sl], p["ens_var"]) and np.array_equal(ua.ensemble_mutual_info[:, sl], p["ens_mutual_info"])
        assert np.array_equal(ua.ensemble_pred_entropy[:, sl], p["ens_pred_entropy"])
    ens = weighted_exit_ensembles(ua.mean, W)
    np.testing.assert_array_equal(ua.ensemble_ape, [average_predictive_entropy(a) for a in ens])
