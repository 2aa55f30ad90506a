"""-m gpu: adaptive Monte-Carlo sampling on the device (bmi_forward_mcd_adaptive / MCDEngine.predict_adaptive) against a fixed run done
step by step with ``accumulate(t_begin = k t_step, t_count = t_step)``: every image's sums equal that run's snapshot at its own t_used bit
for bit (every sample keeps its global index; the compacted steps run the row-table forms of the same kernels), and t_used / converged
equal a float64 numpy re-derivation of the stop rule from the snapshots."""
import time

import numpy as np
import pytest
import torch

from bayesnn_fpga_amd import _lib
from bayesnn_fpga_amd.models import extra as bx
from bayesnn_fpga_amd.models.resnet18.resnet18 import ResNet18MCEarlyExit
from bayesnn_fpga_amd.synthetic import synthetic_images, synthetic_weights_
from tests.helpers import build_seeded

pytestmark = [pytest.mark.gpu, pytest.mark.usefixtures("fp16_engine_default")]
DEV = "cuda:0"

MODELS = {
    "r18_block": (ResNet18MCEarlyExit, dict(dropout_exit=True, dropout="block", dropout_p=0.25, out_dim=10)),
    "r18_layer": (ResNet18MCEarlyExit, dict(dropout_exit=True, dropout="layer", dropout_p=0.25, out_dim=10)),
    "r18_exit_only": (ResNet18MCEarlyExit, dict(dropout_exit=True, dropout=None, dropout_p=0.25, out_dim=10)),
    "r18_masksembles": (ResNet18MCEarlyExit, dict(dropout_exit=True, dropout="block", mask_type="mask", num_masks=4, mask_scale=4.0,
                                                  out_dim=10)),
    "vgg11": (bx.VGG11MC, dict(num_bayes_layer=5)),        # sites in the conv stack (MAXPOOL + MASK) and in the dense layers
    "r50": (bx.ResNet50MCEarlyExit, dict(dropout_exit=True, dropout="block", dropout_p=0.25, out_dim=10)),
}

_ENGINES = {}


def engine(name, dt, B, chunk=None):
    key = (name, dt, B, chunk)
    if key not in _ENGINES:
        cls, kw = MODELS[name]
        m = build_seeded(cls, kw)
        synthetic_weights_(m, 0)
        _ENGINES[key] = m.to(DEV).eval().engine(torch.device(DEV), max_batch=B, chunk_samples=chunk, dtype=dt)
    return _ENGINES[key]


def snapshots(eng, x, T_max, t_step, seed, cnt0=0, with_H=False):
    """The fixed run step by step: {t: (S, H)} after every step (t = samples so far), host float64."""
    B = x.shape[0]
    S, H = eng.new_uncertainty_sums(B) if with_H else (eng.new_moments(B), None)
    out = {}
    for t0 in range(0, T_max, t_step):
        tc = min(t_step, T_max - t0)
        if with_H:
            eng.accumulate_uncertainty(x, S, H, t0, tc, seed, cnt0)
        else:
            eng.accumulate(x, S, t0, tc, seed, cnt0)
        out[t0 + tc] = (S.cpu().numpy().copy(), None if H is None else H.cpu().numpy().copy())
    return out


def stat(S, e, t, rule):
    """The header's statistic of every image at exit e from sums of t samples, float64 [B]."""
    m = S[0, e] / t
    v = np.maximum(S[1, e] / t - m * m, 0.0)
    if rule == "sem":
        return np.sqrt(v / t).max(-1)
    order = np.argsort(-m, axis=-1, kind="stable")
    c1, c2 = order[:, 0], order[:, 1]
    idx = np.arange(m.shape[0])
    d = m[idx, c1] - m[idx, c2]
    den = np.sqrt((v[idx, c1] + v[idx, c2]) / t)
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(den > 0, d / np.where(den > 0, den, 1.0), np.where(d > 0, np.inf, 0.0))
    return r


def passes(s, thr, rule):
    return s <= thr if rule == "sem" else s >= thr


def rederive(snap, e, rule, thr, B):
    """t_used / converged / active_after_step of the rule applied to the snapshots."""
    ts = sorted(snap)
    t_used = np.full(B, ts[-1], dtype=np.int32)
    active = np.ones(B, dtype=bool)
    act = []
    for t in ts:
        ok = passes(stat(snap[t][0], e, t, rule), thr, rule)
        t_used[active] = t
        active &= ~ok
        act.append(int(active.sum()))
        if not active.any():
            break
    act += [0] * (len(ts) - len(act))
    conv = np.array([passes(stat(snap[int(t_used[b])][0], e, int(t_used[b]), rule)[b], thr, rule) for b in range(B)])
    return t_used, conv, act


def pick_threshold(snap, e, rule, q):
    """A midpoint between two observed statistics (of every step), near the q-quantile of the first step's: no image within 1e-9."""
    ts = sorted(snap)
    allv = np.unique(np.concatenate([stat(snap[t][0], e, t, rule) for t in ts]))
    allv = allv[np.isfinite(allv)]
    mids = [(a + b) / 2 for a, b in zip(allv[:-1], allv[1:]) if b - a > 1e-8]
    target = np.quantile(stat(snap[ts[0]][0], e, ts[0], rule)[np.isfinite(stat(snap[ts[0]][0], e, ts[0], rule))], q)
    return float(min(mids, key=lambda v: abs(v - target)))


def check_truncation(eng, x, snap, r_S, r_H, t_used):
    for b in range(x.shape[0]):
        S_ref, H_ref = snap[int(t_used[b])]
        np.testing.assert_array_equal(r_S[:, :, b], S_ref[:, :, b], err_msg=f"image {b} at t_used={int(t_used[b])}")
        if r_H is not None:
            np.testing.assert_array_equal(r_H[:, b], H_ref[:, b])


def run_adaptive(eng, x, T_max, t_step, thr, rule, seed, e=-1, cnt0=0, with_H=False):
    B = x.shape[0]
    S, H = eng.new_uncertainty_sums(B) if with_H else (eng.new_moments(B), None)
    t_used, conv, act = eng.accumulate_adaptive(x, S, T_max, thr, rule, t_step, e, seed, cnt0, H)
    return S.cpu().numpy(), None if H is None else H.cpu().numpy(), t_used.cpu().numpy(), conv.cpu().numpy().astype(bool), act


@pytest.mark.parametrize("dt", ["f16", "bf16", "f16x2", "bf16x3"])
@pytest.mark.parametrize("name", sorted(MODELS))
def test_adaptive_equals_fixed_run_truncated_at_t_used(name, dt):
    B, T_max, t_step, seed = 45, 12, 4, 11
    eng = engine(name, dt, B, chunk=t_step)
    x = synthetic_images(B, seed=21).to(DEV)
    with_H = name == "r18_block"
    snap = snapshots(eng, x, T_max, t_step, seed, with_H=with_H)
    e = eng.n_exits - 1
    for rule, q in (("sem", 0.4), ("margin", 0.6)):
        thr = pick_threshold(snap, e, rule, q)
        S, H, t_used, conv, act = run_adaptive(eng, x, T_max, t_step, thr, rule, seed, with_H=with_H)
        want_t, want_c, want_act = rederive(snap, e, rule, thr, B)
        np.testing.assert_array_equal(t_used, want_t)
        np.testing.assert_array_equal(conv, want_c)
        assert act == want_act
        assert len(set(t_used.tolist())) > 1, f"{rule}: images should retire at more than one step ({act})"
        check_truncation(eng, x, snap, S, H, t_used)


@pytest.mark.parametrize("rule", ["sem", "margin"])
def test_decisions_at_an_inner_exit(rule):
    """test_exit = 1: the rule on exit 1's sums; every exit's rows are still truncated at the same t_used."""
    B, T_max, t_step, seed = 45, 12, 4, 5
    eng = engine("r18_block", "f16", B, chunk=t_step)
    x = synthetic_images(B, seed=22).to(DEV)
    snap = snapshots(eng, x, T_max, t_step, seed)
    thr = pick_threshold(snap, 1, rule, 0.5)
    S, _, t_used, conv, act = run_adaptive(eng, x, T_max, t_step, thr, rule, seed, e=1)
    want_t, want_c, want_act = rederive(snap, 1, rule, thr, B)
    np.testing.assert_array_equal(t_used, want_t)
    np.testing.assert_array_equal(conv, want_c)
    assert act == want_act
    check_truncation(eng, x, snap, S, None, t_used)


def test_nobody_converges_equals_the_fixed_run():
    B, T_max, t_step, seed = 45, 12, 4, 3
    eng = engine("r18_block", "f16", B, chunk=t_step)
    x = synthetic_images(B, seed=23).to(DEV)
    S, _, t_used, conv, act = run_adaptive(eng, x, T_max, t_step, -1.0, "sem", seed)
    assert (t_used == T_max).all() and not conv.any() and act == [B, B, B]
    ref = eng.new_moments(B)
    eng.accumulate(x, ref, 0, T_max, seed)
    np.testing.assert_array_equal(S, ref.cpu().numpy())
    r = eng.predict_adaptive(x, T_max, -1.0, t_step=t_step, seed=seed)
    p = eng.predict(x, T_max, seed=seed)
    for k in ("mean", "var", "logit_mean"):
        assert torch.equal(r[k], p[k])


def test_everybody_converges_after_one_step():
    B, T_max, t_step, seed = 45, 12, 4, 3
    eng = engine("r18_block", "f16", B, chunk=t_step)
    x = synthetic_images(B, seed=23).to(DEV)
    S, _, t_used, conv, act = run_adaptive(eng, x, T_max, t_step, 1e9, "sem", seed)
    assert (t_used == t_step).all() and conv.all() and act == [0, 0, 0]
    snap = snapshots(eng, x, t_step, t_step, seed)
    np.testing.assert_array_equal(S, snap[t_step][0])


def test_no_later_launches_after_everybody_retired():
    """With every image retired after step 1 the engine launches the suffix once: as many suffix launches as one fixed step."""
    B, t_step, seed = 45, 4, 3
    eng = engine("r18_block", "f16", B, chunk=t_step)
    x = synthetic_images(B, seed=23).to(DEV)
    def launches(T_max):
        eng.profile_read()
        run_adaptive(eng, x, T_max, t_step, 1e9, "sem", seed)
        torch.cuda.synchronize()
        eng.profile_read()
        return [(l["kind"], l["images"]) for l in eng.profile_launches()]
    eng.profile(True)
    try:
        n_adaptive, n_one = launches(12), launches(t_step)
    finally:
        eng.profile(False)
    assert n_adaptive == n_one and len(n_one) > 0
    assert all(images in (B, B * t_step) for _, images in n_one)      # prefix (B images) and one full step (t_step x B)


@pytest.mark.parametrize("B,T_max,t_step", [(45, 10, 4), (45, 3, 4), (1, 12, 4), (1, 3, 4)])
def test_ragged_steps_and_tiny_batches(B, T_max, t_step):
    seed = 17
    eng = engine("r18_block", "f16", 45, chunk=t_step)
    x = synthetic_images(B, seed=24).to(DEV)
    snap = snapshots(eng, x, T_max, t_step, seed)
    e = eng.n_exits - 1
    for thr in (pick_threshold(snap, e, "sem", 0.5) if len(snap) > 1 and B > 1 else 1e9, -1.0):
        S, _, t_used, conv, act = run_adaptive(eng, x, T_max, t_step, thr, "sem", seed)
        want_t, want_c, want_act = rederive(snap, e, "sem", thr, B)
        np.testing.assert_array_equal(t_used, want_t)
        np.testing.assert_array_equal(conv, want_c)
        assert act == want_act
        check_truncation(eng, x, snap, S, None, t_used)


def test_image_offset_share_equals_its_rows_of_the_whole_batch():
    B, T_max, t_step, seed, off = 48, 12, 4, 9, 16
    eng = engine("r18_block", "f16", B, chunk=t_step)
    assert eng.image_offset_ok(off)
    x = synthetic_images(B, seed=25).to(DEV)
    snap = snapshots(eng, x, T_max, t_step, seed)
    thr = pick_threshold(snap, eng.n_exits - 1, "sem", 0.5)
    S, _, t_used, conv, _ = run_adaptive(eng, x, T_max, t_step, thr, "sem", seed)
    share = x[off:off + 16].contiguous()
    Ss = eng.new_moments(16)
    tu, cv, _ = eng.accumulate_adaptive(share, Ss, T_max, thr, "sem", t_step, -1, seed, 0, None, off)
    np.testing.assert_array_equal(tu.cpu().numpy(), t_used[off:off + 16])
    np.testing.assert_array_equal(cv.cpu().numpy().astype(bool), conv[off:off + 16])
    np.testing.assert_array_equal(Ss.cpu().numpy(), S[:, :, off:off + 16])


def test_uncertainty_equals_finalize_uncertainty_at_t_used():
    B, T_max, t_step, seed = 45, 12, 4, 7
    eng = engine("r18_block", "f16", B, chunk=t_step)
    x = synthetic_images(B, seed=26).to(DEV)
    snap = snapshots(eng, x, T_max, t_step, seed, with_H=True)
    thr = pick_threshold(snap, eng.n_exits - 1, "sem", 0.4)
    r = eng.predict_adaptive(x, T_max, thr, t_step=t_step, seed=seed, uncertainty=True)
    t_used = r["t_used"].cpu().numpy()
    assert len(set(t_used.tolist())) > 1
    assert r["converged"].dtype == torch.bool and r["t_used"].dtype == torch.int32
    for t in sorted(set(t_used.tolist())):
        S, H = (torch.from_numpy(a).to(DEV) for a in snap[t])
        ref = eng.finalize_uncertainty(S.contiguous(), H.contiguous(), t)
        idx = torch.from_numpy(np.nonzero(t_used == t)[0]).to(DEV)
        for k in ("mean", "var", "logit_mean"):
            assert torch.equal(r[k][:, idx], ref[k][:, idx]), k
        for k in ("pred_entropy", "exp_entropy", "mutual_info"):
            assert torch.equal(r[k][:, idx], ref[k][:, idx]), k
    eng.check_finite()


def test_exact_engine_raises():
    eng = engine("r18_block", "f32", 8, chunk=4)
    x = synthetic_images(8, seed=27).to(DEV)
    with pytest.raises(_lib.BmiError):
        eng.predict_adaptive(x, 8, 0.01, t_step=4)


def test_adaptive_saves_time_at_full_size():
    """Headline model, B = 250, T_max = 100, t_step = 25, a threshold that retires at least half the images after step 1: the adaptive
    call is below 0.85 x fixed predict(T=100) (work fraction <= 0.625)."""
    B, T_max, t_step, seed = 250, 100, 25, 3
    cls, kw = MODELS["r18_block"]
    m = build_seeded(cls, kw)
    synthetic_weights_(m, 0)
    eng = m.to(DEV).eval().engine(torch.device(DEV), max_batch=B)
    x = synthetic_images(B, seed=1234).to(DEV)
    S = eng.new_moments(B)
    eng.accumulate(x, S, 0, t_step, seed)
    s1 = stat(S.cpu().numpy(), eng.n_exits - 1, t_step, "sem")
    thr = float(np.quantile(s1, 0.6))

    def timed(fn):
        fn()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(3):
            fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / 3
    t_fixed = timed(lambda: eng.predict(x, T_max, seed=seed))
    t_adapt = timed(lambda: eng.predict_adaptive(x, T_max, thr, t_step=t_step, seed=seed))
    r = eng.predict_adaptive(x, T_max, thr, t_step=t_step, seed=seed)
    print(f"fixed {t_fixed * 1e3:.2f} ms, adaptive {t_adapt * 1e3:.2f} ms, active after steps {r['active_after_step']}, "
          f"mean t_used {r['t_used'].float().mean().item():.1f}")
    assert r["active_after_step"][0] <= B // 2
    assert t_adapt < 0.85 * t_fixed
