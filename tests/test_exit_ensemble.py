"""-m gpu: the exit ensemble as a predictor on the device (csrc/ensemble.hip: bmi_forward_mcd_ensemble / bmi_finalize_ensemble /
bmi_ensemble_moments) — against the host restatement on the engine's own per-sample logits on every engine type, against the reference's
golden per-pass logits, bit-exact invariance under the split into calls, temperature, the stand-alone entry, the walk, graph capture."""
import numpy as np
import pytest
import torch

from bayesnn_fpga_amd import _lib
from bayesnn_fpga_amd.engine import MCDEngine
from bayesnn_fpga_amd.models.resnet18.resnet18 import ResNet18MCEarlyExit
from bayesnn_fpga_amd.models.vgg19.vgg19 import VGG19MCEarlyExit
from bayesnn_fpga_amd.synthetic import synthetic_images, synthetic_labels, synthetic_weights_
from bayesnn_fpga_amd.train.results_analyzer import exit_ensembles
from bayesnn_fpga_amd.train.uncertainty import UncertaintyAnalysis, decompose_ensemble_logits
from tests.helpers import build_seeded, golden_kwargs, load_golden

pytestmark = [pytest.mark.gpu, pytest.mark.usefixtures("fp16_engine_default")]
DEV = "cuda:0"
DTYPES = ["f16", "bf16", "f32", "f16x2", "bf16x3"]
CONFIGS = ["resnet18_exit_only", "resnet18_block_exit", "resnet18_layer_exit", "resnet18_mask4_block_exit", "resnet18_mask8_exit_c100",
           "vgg19_exit_mc"]
# device name -> decompose_ensemble_logits name, absolute tolerance: float64 on both sides (the device's libm against numpy's: the
# tolerances of tests/test_temperature.py and tests/test_uncertainty.py for device float64 against numpy)
PAIRS = (("ens_mean", "mean", 1e-12), ("ens_var", "var", 1e-12), ("ens_pred_entropy", "pred_entropy", 1e-9),
         ("ens_exp_entropy", "exp_entropy", 1e-9), ("ens_mutual_info", "mutual_info", 1e-9))


def _golden_model(name):
    g = load_golden(f"{name}.npz")
    cls = VGG19MCEarlyExit if name.startswith("vgg19") else ResNet18MCEarlyExit
    m = synthetic_weights_(build_seeded(cls, golden_kwargs(g)), 0).to(DEV).eval()
    x = synthetic_images(int(g["B"]), seed=1234).to(DEV)
    return m, g, x, int(g["T"]), int(g["seed"])


def _np(r):
    return {k: v.cpu().numpy() for k, v in r.items()}


def _check_against_host(r, ref, what=""):
    for dn, hn, tol in PAIRS:
        err = float(np.abs(r[dn] - ref[hn]).max())
        assert err <= tol, f"{what} {dn}: {err:.3e} > {tol:.0e}"


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("name", CONFIGS)
def test_self_consistency_and_untouched_sums(name, dt):
    """predict_ensemble against the host restatement on the SAME engine's per-sample logits; S and H are accumulate_uncertainty's bits;
    ens_mean against exit_ensembles(mean) to 1e-6: the head's softmax is fp32, a probability's absolute error is
    p |z - max| x a few 2^-24 <= 0.37 x 3e-7, and averaging exits does not enlarge it."""
    m, g, x, T, seed = _golden_model(name)
    B = x.shape[0]
    eng = m.engine(x.device, max_batch=B, dtype=dt)
    assert eng.dtype == dt
    S, H, Q, QH = eng.new_ensemble_sums(B)
    assert S._base is H._base is Q._base is QH._base and S._base.numel() == S.numel() + H.numel() + Q.numel() + QH.numel()
    eng.accumulate_ensemble(x, S, H, Q, QH, 0, T, seed, 0)
    r = _np(eng.finalize_ensemble(S, H, Q, QH, T))
    eng.check_finite()
    ref = decompose_ensemble_logits(eng.forward_samples(x, T, seed=seed, cnt0=0).cpu().numpy())
    _check_against_host(r, ref, f"{name}/{dt}")
    S0, H0 = eng.new_uncertainty_sums(B)
    eng.accumulate_uncertainty(x, S0, H0, 0, T, seed, 0)
    assert torch.equal(S, S0) and torch.equal(H, H0)
    np.testing.assert_allclose(r["ens_mean"], exit_ensembles(r["mean"]), rtol=0, atol=1e-6)
    r2 = _np(eng.predict_ensemble(x, T, seed=seed, cnt0=0))
    assert all(np.array_equal(r[k], r2[k]) for k in r)
    assert (r["ens_mutual_info"] >= 0).all() and (r["ens_var"] >= 0).all()


@pytest.mark.parametrize("dt", ["f16", "f16x2"])
@pytest.mark.parametrize("name", CONFIGS)
def test_against_the_reference_goldens(name, dt):
    """With d = max |engine per-pass logits - golden logits| measured here: |ens_mean - ref| <= d/2 + d^2 (first order
    |dp_c| <= 2 d p_c (1 - p_c) <= d/2; averaging exits and samples is a contraction), |ens_var - ref| <= 2 d + 4 d^2 (q, m in [0, 1]:
    |d(q^2)| + |d(m^2)| <= 4 |dq|), the entropies within 6 ln(C) d + d^2 + 1e-9 (tests/test_uncertainty.py:
    test_against_the_reference_goldens derives it per exit; an ensemble member is a mean of such softmaxes).  And the project's own bar:
    1e-3 on ens_mean and ens_var."""
    m, g, x, T, seed = _golden_model(name)
    B = x.shape[0]
    eng = m.engine(x.device, max_batch=B, dtype=dt)
    logits = eng.forward_samples(x, T, seed=seed, cnt0=0).cpu().numpy()
    ref_logits = g["logits"]
    assert logits.shape == ref_logits.shape
    d = float(np.abs(logits.astype(np.float64) - ref_logits).max())
    Cn = ref_logits.shape[-1]
    ref = decompose_ensemble_logits(ref_logits)
    r = _np(eng.predict_ensemble(x, T, seed=seed, cnt0=0))
    eng.check_finite()
    err = {dn: float(np.abs(r[dn] - ref[hn]).max()) for dn, hn, _ in PAIRS}
    print(f"{name}/{dt}: d = {d:.3e} " + " ".join(f"{k} {v:.3e}" for k, v in err.items()))
    assert err["ens_mean"] <= d / 2 + d * d, f"ens_mean {err['ens_mean']:.3e} (d = {d:.3e})"
    assert err["ens_var"] <= 2 * d + 4 * d * d, f"ens_var {err['ens_var']:.3e} (d = {d:.3e})"
    bound = 6 * np.log(Cn) * d + d * d + 1e-9
    for q in ("ens_pred_entropy", "ens_exp_entropy", "ens_mutual_info"):
        assert err[q] <= bound, f"{q}: {err[q]:.3e} > {bound:.3e} (d = {d:.3e})"
    assert err["ens_mean"] <= 1e-3 and err["ens_var"] <= 1e-3, f"the 1e-3 bar: ens_mean {err['ens_mean']:.3e}, ens_var {err['ens_var']:.3e}"


def _sums(eng, x, T, seed, t_ranges=None, shares=None):
    B = x.shape[0]
    S, H, Q, QH = eng.new_ensemble_sums(B)
    if shares:
        for lo, hi in shares:
            part = eng.new_ensemble_sums(hi - lo)
            eng.accumulate_ensemble(x[lo:hi], *part, 0, T, seed, 0, image_offset=lo)
            Q[:, :, lo:hi] += part[2]
            QH[:, lo:hi] += part[3]
    else:
        for t0, n in (t_ranges or [(0, T)]):
            eng.accumulate_ensemble(x, S, H, Q, QH, t0, n, seed, 0)
    return Q.cpu().numpy(), QH.cpu().numpy()


@pytest.mark.parametrize("kw", [dict(dropout_exit=True, dropout=None, dropout_p=0.25, out_dim=100),
                                dict(dropout_exit=True, dropout="block", dropout_p=0.25, out_dim=10),
                                dict(dropout_exit=True, dropout="block", dropout_p=0.25, out_dim=10, mask_type="mask", num_masks=4,
                                     mask_scale=4.0)], ids=["exit_only_c100", "block", "mask4"])
def test_invariance_under_the_split_into_calls(kw):
    """Q and QH are one running sum per (exit, image, class) continued in sample order: t-ranges accumulated into one buffer give the BITS
    of one call; image shares give the bits of their rows (zero + the share's sum); two t-shards summed from separate zeroed buffers to
    rtol 1e-12 (a different association).  An engine planned with chunk_samples=32 against the default one: bit for bit where the
    per-sample logits do not depend on the plan — exit-only dropout on fp16; with convs in the suffix the planned chunk picks the fp16
    engine's conv kernels (tests/test_uncertainty.py: test_invariance_chunks_tshards_image_shares_and_head_batch), so the two plans are
    compared on f16x2."""
    B, T, seed = 8, 70, 11
    model = synthetic_weights_(build_seeded(ResNet18MCEarlyExit, kw), 0).to(DEV).eval()
    x = synthetic_images(B, seed=77).to(DEV)
    e_def = MCDEngine(model, DEV, max_batch=B)
    assert e_def.chunk_samples >= T
    Q, QH = _sums(e_def, x, T, seed)
    assert (QH > 0).all() and (Q[0] > 0).any()
    for ranges in ([(0, 32), (32, 32), (64, T - 64)], [(0, 29), (29, T - 29)]):
        Q2, QH2 = _sums(e_def, x, T, seed, t_ranges=ranges)
        assert np.array_equal(Q2, Q) and np.array_equal(QH2, QH), ranges
    Qa, QHa = _sums(e_def, x, T, seed, t_ranges=[(0, 29)])
    Qb, QHb = _sums(e_def, x, T, seed, t_ranges=[(29, T - 29)])
    np.testing.assert_allclose(Qa + Qb, Q, rtol=1e-12, atol=0)
    np.testing.assert_allclose(QHa + QHb, QH, rtol=1e-12, atol=0)
    Qs, QHs = _sums(e_def, x, T, seed, shares=[(0, 4), (4, 8)])
    assert np.array_equal(Qs, Q) and np.array_equal(QHs, QH)
    dt = "f16" if kw["dropout"] is None else "f16x2"
    p_def, p32 = MCDEngine(model, DEV, max_batch=B, dtype=dt), MCDEngine(model, DEV, max_batch=B, chunk_samples=32, dtype=dt)
    assert p32.chunk_samples == 32 < T <= p_def.chunk_samples
    l_def, l32 = p_def.forward_samples(x, T, seed=seed), p32.forward_samples(x, T, seed=seed)
    assert torch.equal(l_def, l32), "the caveat this comparison stands on: the two plans give the same per-sample logits"
    Qd, QHd = _sums(p_def, x, T, seed)
    Q32, QH32 = _sums(p32, x, T, seed)
    assert np.array_equal(Q32, Qd) and np.array_equal(QH32, QHd)


@pytest.mark.parametrize("name", ["resnet18_block_exit", "resnet18_mask8_exit_c100", "vgg19_exit_mc"])
def test_temperature(name):
    m, g, x, T, seed = _golden_model(name)
    B = x.shape[0]
    eng = m.engine(x.device, max_batch=B, dtype="f16x2")
    plain = _np(eng.predict_ensemble(x, T, seed=seed))
    logits = eng.forward_samples(x, T, seed=seed).cpu().numpy()
    tau = [0.6 + 0.45 * e for e in range(eng.n_exits)]
    eng.set_temperature(tau)
    try:
        r = _np(eng.predict_ensemble(x, T, seed=seed))
        eng.check_finite()
        assert np.array_equal(eng.forward_samples(x, T, seed=seed).cpu().numpy(), logits)      # raw logits stay raw
        _check_against_host(r, decompose_ensemble_logits(logits, tau), f"{name} tempered")
        assert np.abs(r["ens_mean"] - plain["ens_mean"]).max() > 1e-3
        np.testing.assert_allclose(r["ens_mean"], exit_ensembles(r["mean"]), rtol=0, atol=1e-6)
        eng.set_temperature([1.0] * eng.n_exits)
        ones = _np(eng.predict_ensemble(x, T, seed=seed))
        assert all(np.array_equal(ones[k], plain[k]) for k in plain)
    finally:
        eng.set_temperature(None)


def _any_engine():
    kw = dict(dropout_exit=True, dropout=None, dropout_p=0.25, out_dim=10)
    model = synthetic_weights_(build_seeded(ResNet18MCEarlyExit, kw), 0).to(DEV).eval()
    return MCDEngine(model, DEV, max_batch=2)


@pytest.mark.parametrize("shape", [(1, 1, 1, 2), (7, 4, 3, 10), (33, 5, 9, 100), (100, 4, 16, 10), (10, 4, 250, 100), (3, 2, 5, 128)],
                         ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("scale", [1.0, 100.0], ids=["random", "peaky"])
def test_stand_alone_entry(shape, scale):
    T, E, B, Cn = shape
    eng = _any_engine()
    g = torch.Generator().manual_seed(T * 1000 + Cn)
    logits = (torch.randn(T, E, B, Cn, generator=g) * scale).to(DEV)
    r = eng.ensemble_moments(logits)
    eng.check_finite()
    rn = _np(r)
    assert all(np.isfinite(v).all() for v in rn.values())
    _check_against_host(rn, decompose_ensemble_logits(logits.cpu().numpy()), str(shape))
    again = eng.ensemble_moments(logits)
    assert all(torch.equal(r[k], again[k]) for k in r)
    if T >= 2:
        h = T // 2
        first = eng.ensemble_moments(logits[:h].contiguous())
        both = eng.ensemble_moments(logits[h:].contiguous(), out=(first["Q"], first["QH"]), t_before=h)
        assert all(torch.equal(r[k], both[k]) for k in r)
    tau = [0.5 + 0.7 * e for e in range(E)]
    rt = _np(eng.ensemble_moments(logits, tau=tau))
    _check_against_host(rt, decompose_ensemble_logits(logits.cpu().numpy(), tau), f"{shape} tempered")
    ones = eng.ensemble_moments(logits, tau=1.0)
    assert all(torch.equal(r[k], ones[k]) for k in r)


def test_stand_alone_entry_refuses_what_the_kernel_does_not_take():
    import ctypes as C
    lib = _lib.lib()
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    for T, E, B, Cn in ((2, 2, 2, 129), (2, 33, 2, 10), (2, 32, 2, 128)):
        logits = torch.zeros(T, E, B, Cn, device=DEV)
        Q = torch.zeros(2, E, B, Cn, dtype=torch.float64, device=DEV)
        QH = torch.zeros(E, B, dtype=torch.float64, device=DEV)
        rc = lib.bmi_ensemble_moments(logits.data_ptr(), T, E, B, Cn, None, Q[0].data_ptr(), Q[1].data_ptr(), QH.data_ptr(), st)
        assert rc == -95, (T, E, B, Cn, rc)
        assert not Q.any() and not QH.any()
    logits = torch.zeros(2, 2, 2, 10, device=DEV)
    Q = torch.zeros(2, 2, 2, 10, dtype=torch.float64, device=DEV)
    QH = torch.zeros(2, 2, dtype=torch.float64, device=DEV)
    bad = (C.c_float * 2)(1.0, 0.0)
    assert lib.bmi_ensemble_moments(logits.data_ptr(), 2, 2, 2, 10, bad, Q[0].data_ptr(), Q[1].data_ptr(), QH.data_ptr(), st) == -22
    assert lib.bmi_ensemble_moments(None, 2, 2, 2, 10, None, Q[0].data_ptr(), Q[1].data_ptr(), QH.data_ptr(), st) == -22


def test_forward_entry_checks_its_scratch_before_any_launch():
    import ctypes as C
    eng = _any_engine()
    B = 2
    x = synthetic_images(B, seed=5).to(DEV)
    S, H, Q, QH = eng.new_ensemble_sums(B)
    need = int(eng.lib.bmi_ensemble_scratch_bytes(eng.handle, B))
    assert need == eng.chunk_samples * eng.n_exits * B * eng.out_dim * 4
    assert int(eng.lib.bmi_ensemble_scratch_bytes(eng.handle, eng.max_batch + 1)) == 0
    small = torch.empty(need - 4, dtype=torch.uint8, device=DEV)

    def call(scratch, nbytes, q1):
        return eng.lib.bmi_forward_mcd_ensemble(eng.handle, x.data_ptr(), B, 0, 0, 3, 1, 0, S[0].data_ptr(), S[1].data_ptr(), S[2].data_ptr(),
                                                H.data_ptr(), q1, Q[1].data_ptr(), QH.data_ptr(), scratch, nbytes, eng.workspace.data_ptr(),
                                                eng.workspace_bytes, C.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert call(small.data_ptr(), small.numel(), Q[0].data_ptr()) == -12          # BMI_ERR_NOMEM
    assert call(None, need, Q[0].data_ptr()) == -22 and call(small.data_ptr(), need, None) == -22        # BMI_ERR_INVALID
    torch.cuda.synchronize()
    assert not S._base.any()


def test_finalize_ensemble_counts_nonfinite_sums():
    eng = _any_engine()
    logits = torch.randn(3, 2, 4, 10, generator=torch.Generator().manual_seed(1)).to(DEV)
    logits[1, 1, 2, 3] = float("nan")
    assert eng.nonfinite_count() == 0
    r = _np(eng.ensemble_moments(logits))
    assert eng.nonfinite_count() == 10 + 1                # the row's classes (an element counts once, like bmi_finalize_checked) and its QH
    assert np.isnan(r["ens_mean"][1, 2]).all() and np.isnan(r["ens_mutual_info"][1, 2]) and np.isnan(r["ens_var"][1, 2]).all()
    ok = np.ones((2, 4), bool)
    ok[1, 2] = False
    assert np.isfinite(r["ens_mean"][ok]).all() and np.isfinite(r["ens_exp_entropy"][ok]).all()
    with pytest.raises(FloatingPointError):
        eng.ensemble_moments(logits)
        eng.check_finite()


@pytest.mark.parametrize("kw", [dict(dropout_exit=True, dropout="block", dropout_p=0.25, out_dim=10),
                                dict(dropout_exit=True, dropout="block", dropout_p=0.25, out_dim=10, mask_type="mask", num_masks=4,
                                     mask_scale=4.0)], ids=["mc", "mask4"])
def test_uncertainty_analysis_with_ensembles(kw, tmp_path, monkeypatch):
    m = synthetic_weights_(build_seeded(ResNet18MCEarlyExit, kw), 0).to(DEV).eval()
    B, T, seed = 4, 10, 7
    x, y = synthetic_images(3 * B, seed=3), synthetic_labels(3 * B, 10, seed=4)
    loader = [(x[i * B:(i + 1) * B], y[i * B:(i + 1) * B]) for i in range(3)]
    ml = m.mask_layers()
    cnt_start = [l.cnt for l in ml]
    ua0 = UncertaintyAnalysis(m, loader, gpu=0, mc_passes=T, seed=seed)
    cnt_end = [l.cnt for l in ml]
    for l, c in zip(ml, cnt_start):
        l.cnt = c
    ua = UncertaintyAnalysis(m, loader, gpu=0, mc_passes=T, seed=seed, ensemble=True)
    assert [l.cnt for l in ml] == cnt_end
    for q in ("mean", "pred_entropy", "exp_entropy", "mutual_info", "ape", "mean_mi", "ensemble_ape"):
        assert np.array_equal(getattr(ua, q), getattr(ua0, q)), q
    np.testing.assert_allclose(ua.ensemble_pred_entropy, ua0.ensemble_pred_entropy, rtol=0, atol=1e-5)
    assert not hasattr(ua0, "ensemble_var") and "ensemble_mean_mi" not in ua0.summary()[0]
    # the new arrays are the per-batch predict_ensemble results
    eng = m.engine(torch.device(DEV), max_batch=B)
    for l, c in zip(ml, cnt_start):
        l.cnt = c
    for k, (bx, _) in enumerate(loader):
        cnt0 = ml[0].cnt if ml else 0
        m.advance(T)
        r = _np(eng.predict_ensemble(bx.to(DEV), T, seed + k, cnt0=cnt0))
        sl = slice(k * B, (k + 1) * B)
        assert np.array_equal(ua.ensemble_var[:, sl], r["ens_var"])
        assert np.array_equal(ua.ensemble_pred_entropy[:, sl], r["ens_pred_entropy"])
        assert np.array_equal(ua.ensemble_exp_entropy[:, sl], r["ens_exp_entropy"])
        assert np.array_equal(ua.ensemble_mutual_info[:, sl], r["ens_mutual_info"])
    E = ua.mean.shape[0]
    assert ua.ensemble_var.shape == (E, 3 * B, 10) and ua.ensemble_mutual_info.shape == (E, 3 * B)
    assert (ua.ensemble_mutual_info > 0).any()
    np.testing.assert_array_equal(ua.ensemble_mean_mi, ua.ensemble_mutual_info.mean(1))
    assert [d["ensemble_mean_mi"] for d in ua.summary()] == [float(v) for v in ua.ensemble_mean_mi]
    monkeypatch.chdir(tmp_path)
    f = np.load(ua.save("ens"))
    for q in ("ensemble_var", "ensemble_exp_entropy", "ensemble_mutual_info", "ensemble_mean_mi", "ensemble_pred_entropy", "mutual_info"):
        np.testing.assert_array_equal(f[q], getattr(ua, q))
    f0 = np.load(ua0.save("plain"))
    assert set(f0.files) == {"mean", "pred_entropy", "exp_entropy", "mutual_info", "labels", "ape", "mean_mi", "mean_exp_entropy",
                             "ensemble_pred_entropy", "ensemble_ape"}
    assert set(f.files) == set(f0.files) | {"ensemble_var", "ensemble_exp_entropy", "ensemble_mutual_info", "ensemble_mean_mi"}


def test_hipgraph_capture_and_replay():
    """bmi_forward_mcd_ensemble neither allocates nor synchronises (the scratch belongs to the engine from the warm-up on): a captured
    predict replays on new inputs to the eager bits."""
    kw = dict(dropout_exit=True, dropout="block", dropout_p=0.25, out_dim=10)
    model = synthetic_weights_(build_seeded(ResNet18MCEarlyExit, kw), 0).to(DEV).eval()
    B, T, seed = 4, 6, 21
    eng = model.engine(torch.device(DEV), max_batch=B)
    x_static = synthetic_images(B, seed=1).to(DEV)
    S, H, Q, QH = eng.new_ensemble_sums(B)
    out_static = {}
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):                      # warm-up on the capture stream (module load, first launches, the scratch)
        eng.accumulate_ensemble(x_static, S, H, Q, QH, 0, T, seed)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        S._base.zero_()
        eng.accumulate_ensemble(x_static, S, H, Q, QH, 0, T, seed)
        out_static.update(eng.finalize_ensemble(S, H, Q, QH, T))
    for s in (2, 3):
        x_new = synthetic_images(B, seed=s).to(DEV)
        x_static.copy_(x_new)
        graph.replay()
        torch.cuda.synchronize()
        got = {k: v.clone() for k, v in out_static.items()}
        want = eng.predict_ensemble(x_new, T, seed=seed)
        assert set(got) == set(want)
        for k in want:
            assert torch.equal(got[k], want[k]), k
    eng.check_finite()
