"""-m gpu: early exit by stages (bmi_forward_mcd_exit_staged / MCDEngine.predict_early_exit) against the same engine's full run
(``accumulate_uncertainty``, same seed): the decisions equal a float64 numpy restatement of the rule on the full run's sums, every row the
staged call computes equals the full run's bit for bit (S1 / S2 / SL / SH), rows of exits an image never reached stay zero, and the later
stages really run on the active images only."""
import numpy as np
import pytest
import torch

from bayesnn_fpga_amd import _lib
from bayesnn_fpga_amd.models.resnet18.resnet18 import ResNet18MCEarlyExit
from bayesnn_fpga_amd.models.vgg19.vgg19 import VGG19MCEarlyExit
from bayesnn_fpga_amd.synthetic import synthetic_images, synthetic_weights_
from bayesnn_fpga_amd.train import confidence_exiting as cex
from tests.helpers import build_seeded

pytestmark = [pytest.mark.gpu, pytest.mark.usefixtures("fp16_engine_default")]
DEV = "cuda:0"

EXIT_ONLY = dict(dropout_exit=True, dropout=None, dropout_p=0.25, out_dim=100)
MODELS = {
    "r18_exit_only": (ResNet18MCEarlyExit, EXIT_ONLY),
    "vgg19_exit_only": (VGG19MCEarlyExit, EXIT_ONLY),
    "r18_block_exit": (ResNet18MCEarlyExit, dict(dropout_exit=True, dropout="block", dropout_p=0.25, out_dim=10)),
    "r18_masksembles": (ResNet18MCEarlyExit, dict(dropout_exit=True, dropout="block", mask_type="mask", num_masks=4, mask_scale=4.0, out_dim=10)),
}
RULES = [("confidence", False), ("margin", False), ("confidence", True), ("margin", True)]


def _engine(name, dt, B, chunk=None):
    cls, kw = MODELS[name]
    m = build_seeded(cls, kw)
    synthetic_weights_(m, 0)
    return m.to(DEV).eval().engine(torch.device(DEV), max_batch=B, chunk_samples=chunk, dtype=dt)


def _full(eng, x, T, seed):
    S, H = eng.new_uncertainty_sums(x.shape[0])
    eng.accumulate_uncertainty(x, S, H, 0, T, seed)
    return S.cpu().numpy().copy(), H.cpu().numpy().copy()


def _stat(S1, T, rule, ensemble):
    """float64 [E, B]: the rule's statistic per exit, in the kernel's order (per exit: S1 / T; ensembled: the exits' S1 / T summed in exit
    order, / (e + 1))."""
    p = S1 / T
    if ensemble:
        acc = np.zeros_like(p[0])
        ens = []
        for e in range(p.shape[0]):
            acc = acc + p[e]
            ens.append(acc / (e + 1))
        p = np.stack(ens)
    top = -np.sort(-p, axis=2)
    return top[:, :, 0] - top[:, :, 1] if rule == "margin" else top[:, :, 0]


def _decide(stat, thr, first_exit):
    E, B = stat.shape
    out = np.full(B, E - 1)
    for b in range(B):
        for e in range(first_exit, E - 1):
            if stat[e, b] > thr:
                out[b] = e
                break
    return out


def _check_call(eng, x, T, seed, S_full, H_full, rule, ensemble, thr, first_exit=1):
    B, E = x.shape[0], eng.n_exits
    want = _decide(_stat(S_full[0], T, rule, ensemble), thr, first_exit)
    S, H = eng.new_uncertainty_sums(B)
    xl, act = eng.accumulate_early_exit(x, S, T, thr, seed=seed, first_exit=first_exit, rule=rule, ensemble=ensemble, H=H)
    got = xl.cpu().numpy()
    np.testing.assert_array_equal(got, want)
    S, H = S.cpu().numpy(), H.cpu().numpy()
    for e in range(E):
        reached = got >= e
        np.testing.assert_array_equal(S[:, e][:, reached], S_full[:, e][:, reached])
        np.testing.assert_array_equal(H[e][reached], H_full[e][reached])
        assert not S[:, e][:, ~reached].any() and not H[e][~reached].any()
    exp_act = [B if e < first_exit else int((got > e).sum()) for e in range(E - 1)] + [int((got == E - 1).sum())]
    assert act == exp_act
    return got, act


@pytest.mark.parametrize("dt", ["f16", "bf16", "f16x2", "bf16x3"])
@pytest.mark.parametrize("name", sorted(MODELS))
def test_staged_exit_equals_the_full_run_bit_for_bit(name, dt):
    B, T, seed = 45, 6, 11
    eng = _engine(name, dt, B)
    x = synthetic_images(B, seed=21).to(DEV)
    S_full, H_full = _full(eng, x, T, seed)
    for rule, ens in RULES:
        stat = _stat(S_full[0], T, rule, ens)
        thrs = [float(np.quantile(stat[1], q)) for q in (0.25, 0.5, 0.75)] + [-1.0, 2.0]
        for thr in thrs:
            got, act = _check_call(eng, x, T, seed, S_full, H_full, rule, ens, thr)
            if thr == -1.0:
                assert (got == 1).all() and act[1] == 0 and act[-1] == 0          # everybody left at the first tested exit
            if thr == 2.0:
                assert (got == eng.n_exits - 1).all() and act[-1] == B


def test_per_exit_confidence_rule_is_the_references():
    """The per-exit confidence rule is cex.exit_layer (the reference's is_confident loop from exit 1) on the full run's means; the margin
    rule is confident(diff=True)."""
    B, T, seed = 45, 6, 5
    eng = _engine("r18_exit_only", "f16", B)
    x = synthetic_images(B, seed=3).to(DEV)
    S_full, _ = _full(eng, x, T, seed)
    p = S_full[0] / T
    for diff, rule in ((False, "confidence"), (True, "margin")):
        stat = _stat(S_full[0], T, rule, False)
        thr = float(np.median(stat[1]))
        r = eng.predict_early_exit(x, T, thr, seed=seed, rule=rule)
        np.testing.assert_array_equal(r["exit_layer"].cpu().numpy(), cex.exit_layer(p.copy(), thr, diff=diff))


def test_predict_early_exit_outputs_and_accounting():
    B, T, seed = 45, 6, 7
    eng = _engine("r18_exit_only", "f16", B)
    x = synthetic_images(B, seed=8).to(DEV)
    full = eng.predict_uncertainty(x, T, seed=seed)
    st = eng.exit_stages(1)
    stat = _stat(_full(eng, x, T, seed)[0][0], T, "confidence", True)
    for thr in (-1.0, float(np.median(stat[1])), 2.0):
        r = eng.predict_early_exit(x, T, thr, seed=seed, ensemble=True, uncertainty=True)
        xl = r["exit_layer"].cpu().numpy()
        mean = full["mean"].cpu().numpy()
        ens = np.cumsum(mean, axis=0) / np.arange(1, eng.n_exits + 1)[:, None, None]
        np.testing.assert_allclose(r["best_preds"].cpu().numpy(), ens[xl, np.arange(B)], rtol=0, atol=1e-13)
        for k in ("pred_entropy", "exp_entropy", "mutual_info"):
            got, want = r[k].cpu().numpy(), full[k].cpu().numpy()
            for e in range(eng.n_exits):
                np.testing.assert_array_equal(got[e][xl >= e], want[e][xl >= e])
        ran = [B] + [r["active_after"][k] for k in range(1, len(st))]
        want_done = sum(n * (s["prefix_macs"] - s["whole_batch_macs"] + T * s["suffix_macs"]) + (B if n else 0) * s["whole_batch_macs"]
                        for n, s in zip(ran, st))
        assert r["macs_done"] == want_done and r["macs_full"] == B * (eng.prefix_macs + T * eng.suffix_macs)
        if thr == 2.0:
            assert r["macs_done"] == r["macs_full"]
        if thr == -1.0:
            assert r["macs_done"] == B * (st[0]["prefix_macs"] + T * st[0]["suffix_macs"]) < r["macs_full"]


@pytest.mark.parametrize("name", ["r18_exit_only", "vgg19_exit_only"])
def test_later_stages_run_on_the_active_images(name):
    """With profiling on, every launch carries the whole batch (stage 0, and the ops the plan marks as whole-batch), or Bc (a later stage's
    prefix op), or T x Bc (its suffix ops), with Bc the images still active; a stage launches at least its row-table ops at Bc / T x Bc."""
    B, T, seed = 45, 6, 11
    eng = _engine(name, "f16", B)
    x = synthetic_images(B, seed=21).to(DEV)
    S_full, _ = _full(eng, x, T, seed)
    stat = _stat(S_full[0], T, "confidence", False)
    fe = 1
    st = eng.exit_stages(fe)
    thr = float(np.quantile(stat[1], 0.4))
    eng.profile(True)
    try:
        r = eng.predict_early_exit(x, T, thr, seed=seed)
        torch.cuda.synchronize()
        eng.profile_read()
        launches = eng.profile_launches()
    finally:
        eng.profile(False)
    act = r["active_after"]
    bcs = [act[fe + k - 1] for k in range(1, len(st)) if act[fe + k - 1] > 0]
    assert bcs and bcs[0] < B
    allowed = {B, T * B} | set(bcs) | {T * b for b in bcs}
    imgs = [ln["images"] for ln in launches]
    assert set(imgs) <= allowed
    for k in range(1, len(st)):
        bc = act[fe + k - 1]
        if bc in (0, B):
            continue
        assert sum(i in (bc, T * bc) for i in imgs) >= st[k]["n_ops"] - st[k]["n_whole_batch_ops"]


@pytest.mark.parametrize("dt", ["f16", "f16x2"])
@pytest.mark.parametrize("name", ["r18_exit_only", "vgg19_exit_only"])
def test_staged_exit_at_the_benchmark_batch(name, dt):
    """B = 250: the prefix launches behind a decision take the large-grid kernels (conv3x3_pw, conv3x3_s2, the wide tiles, split-K on
    VGG's 2x2 maps) under a row table; first_exit 0 also puts layer2's 16x16 convs behind a decision."""
    B, T, seed = 250, 4, 17
    eng = _engine(name, dt, B, chunk=4)
    x = synthetic_images(B, seed=5).to(DEV)
    S_full, H_full = _full(eng, x, T, seed)
    for rule, ens in (("confidence", False), ("margin", True)):
        stat = _stat(S_full[0], T, rule, ens)
        for fe in (0, 1):
            for q in (0.3, 0.7):
                _check_call(eng, x, T, seed, S_full, H_full, rule, ens, float(np.quantile(stat[fe], q)), first_exit=fe)


def test_staged_exit_masksembles_with_a_mask_offset():
    B, T, seed, cnt0 = 45, 6, 11, 3
    eng = _engine("r18_masksembles", "f16", B)
    x = synthetic_images(B, seed=21).to(DEV)
    S, H = eng.new_uncertainty_sums(B)
    eng.accumulate_uncertainty(x, S, H, 0, T, seed, cnt0)
    S_full, H_full = S.cpu().numpy(), H.cpu().numpy()
    stat = _stat(S_full[0], T, "confidence", False)
    for fe in (0, 1):
        thr = float(np.median(stat[fe]))
        want = _decide(stat, thr, fe)
        S2, H2 = eng.new_uncertainty_sums(B)
        xl, _ = eng.accumulate_early_exit(x, S2, T, thr, seed=seed, cnt0=cnt0, first_exit=fe, H=H2)
        got = xl.cpu().numpy()
        np.testing.assert_array_equal(got, want)
        S2, H2 = S2.cpu().numpy(), H2.cpu().numpy()
        for e in range(eng.n_exits):
            np.testing.assert_array_equal(S2[:, e][:, got >= e], S_full[:, e][:, got >= e])
            np.testing.assert_array_equal(H2[e][got >= e], H_full[e][got >= e])


@pytest.mark.parametrize("dt", ["f16", "f16x2"])
def test_vgg19_split_k_runs_compacted(dt):
    """VGG-19 at B = 250 plans split-K for its 2x2-map convs (the last stage): behind a decision those launches carry only the active
    images (conv_igemm / conv_split's row-table split-K form), and repeated calls give the same bits (the partial sums are per K range,
    added in a fixed order)."""
    B, T, seed = 250, 4, 3
    eng = _engine("vgg19_exit_only", dt, B, chunk=4)
    x = synthetic_images(B, seed=2).to(DEV)
    S_full, H_full = _full(eng, x, T, seed)
    stat = _stat(S_full[0], T, "confidence", False)
    thr = float(np.quantile(stat[1], 0.5))
    eng.profile(True)
    try:
        got, act = _check_call(eng, x, T, seed, S_full, H_full, "confidence", False, thr)
        torch.cuda.synchronize()
        eng.profile_read()
        launches = eng.profile_launches()
    finally:
        eng.profile(False)
    bc_last = act[eng.n_exits - 2]
    assert 0 < bc_last < B
    fam = "conv_split" if dt == "f16x2" else "conv_igemm"
    # split-K launches take one profile record each (main kernel + finishing pass); the full run's would carry B images
    sk = [ln for ln in launches if ln["family"] == fam and ln["images"] == bc_last]
    assert len(sk) >= 2, [(ln["family"], ln["images"]) for ln in launches]
    assert all(ln["images"] != B for ln in launches if ln["family"] == fam and ln["out"] in {l2["out"] for l2 in sk})
    for _ in range(10):
        _check_call(eng, x, T, seed, S_full, H_full, "confidence", False, thr)


@pytest.mark.parametrize("B,chunk", [(1, None), (4, None), (11, None), (45, 6)])
def test_staged_exit_on_small_batches(B, chunk):
    T, seed = 6, 3
    eng = _engine("r18_exit_only", "f16", B, chunk)
    x = synthetic_images(B, seed=9).to(DEV)
    S_full, H_full = _full(eng, x, T, seed)
    for rule, ens in (("confidence", False), ("margin", True)):
        stat = _stat(S_full[0], T, rule, ens)
        for thr in (float(np.median(stat[1])), float(np.median(stat[2])), -1.0, 2.0):
            _check_call(eng, x, T, seed, S_full, H_full, rule, ens, thr)
    if B > 1:      # a smaller batch than planned runs the planned batch's kernels
        xs = x[: B - 1].contiguous()
        S_s, H_s = _full(eng, xs, T, seed)
        _check_call(eng, xs, T, seed, S_s, H_s, "confidence", False, float(np.median(_stat(S_s[0], T, "confidence", False)[1])))


def test_staged_exit_is_refused_by_the_exact_engine():
    B = 4
    eng = _engine("r18_exit_only", "f32", B)
    x = synthetic_images(B, seed=1).to(DEV)
    with pytest.raises(_lib.BmiError):
        eng.predict_early_exit(x, 4, 0.5)
    with pytest.raises(ValueError):
        eng.predict_early_exit(x, eng.chunk_samples + 1, 0.5)
