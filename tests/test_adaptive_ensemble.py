"""-m gpu: the exit-ensemble read-out under adaptive sampling (bmi_forward_mcd_adaptive_ensemble / bmi_finalize_ensemble_per_image;
MCDEngine.accumulate_adaptive / predict_adaptive with ``ensemble=True``) against a fixed run done step by step with
``accumulate_ensemble(t_begin = k t_step, t_count = t_step)``: every image's S / H / Q / QH equal that run's snapshot at its own t_used bit
for bit (the image-list form of csrc/ensemble.hip continues the same running sums), and with ``stop_on="ensemble"`` t_used / converged /
active_after_step equal a float64 numpy re-derivation of the stop rule from the Q snapshots (tests/test_adaptive_sampling.py's, which
takes any [2+, E, B, C] pair of sums)."""
import ctypes as C

import numpy as np
import pytest
import torch

from bayesnn_fpga_amd import _lib
from bayesnn_fpga_amd.models.resnet18.resnet18 import ResNet18MCEarlyExit
from bayesnn_fpga_amd.models.vgg19.vgg19 import VGG19MCEarlyExit
from bayesnn_fpga_amd.synthetic import synthetic_images, synthetic_weights_
from bayesnn_fpga_amd.train.uncertainty import decompose_ensemble_logits
from tests.helpers import build_seeded
from tests.test_adaptive_sampling import pick_threshold, rederive
from tests.test_exit_ensemble import PAIRS

pytestmark = [pytest.mark.gpu, pytest.mark.usefixtures("fp16_engine_default")]
DEV = "cuda:0"
B, T_MAX, T_STEP = 45, 12, 4

MODELS = {
    "r18_block": (ResNet18MCEarlyExit, dict(dropout_exit=True, dropout="block", dropout_p=0.25, out_dim=10)),
    # C > 64: the strided class loop of the kernel's 64-lane groups
    "r18_exit_only_c100": (ResNet18MCEarlyExit, dict(dropout_exit=True, dropout=None, dropout_p=0.25, out_dim=100)),
    "r18_masksembles": (ResNet18MCEarlyExit, dict(dropout_exit=True, dropout="block", mask_type="mask", num_masks=4, mask_scale=4.0,
                                                  out_dim=10)),
    "vgg19": (VGG19MCEarlyExit, dict(dropout_exit=True, dropout=None, dropout_p=0.25, out_dim=10)),       # five exits
}
DTYPES = ["f16", "f16x2"]
RULES = (("sem", 0.4), ("margin", 0.6))

_ENGINES = {}
_SNAPS = {}


def engine(name, dt, max_batch=B, chunk=T_STEP):
    key = (name, dt, max_batch, chunk)
    if key not in _ENGINES:
        cls, kw = MODELS[name]
        m = synthetic_weights_(build_seeded(cls, kw), 0)
        _ENGINES[key] = m.to(DEV).eval().engine(torch.device(DEV), max_batch=max_batch, chunk_samples=chunk, dtype=dt)
    return _ENGINES[key]


def snapshots(eng, x, seed, key=None, T_max=T_MAX, t_step=T_STEP):
    """The fixed run step by step: {t: (S, H, Q, QH)} after every step (t = samples so far), host float64.  Computed once per key."""
    if key is not None and key in _SNAPS:
        return _SNAPS[key]
    sums = eng.new_ensemble_sums(x.shape[0])
    out = {}
    for t0 in range(0, T_max, t_step):
        tc = min(t_step, T_max - t0)
        eng.accumulate_ensemble(x, *sums, t0, tc, seed, 0)
        out[t0 + tc] = tuple(a.cpu().numpy().copy() for a in sums)
    if key is not None:
        _SNAPS[key] = out
    return out


def q_sums(snap):
    """{t: (Q,)}: what tests/test_adaptive_sampling.py's stat / rederive / pick_threshold read as (S1, S2) = (Q[0], Q[1])."""
    return {t: (v[2],) for t, v in snap.items()}


def run(eng, x, thr, rule, seed, stop_on, test_exit=-1, image_offset=0):
    sums = eng.new_ensemble_sums(x.shape[0])
    S, H, Q, QH = sums
    t_used, conv, act = eng.accumulate_adaptive(x, S, T_MAX, thr, rule, T_STEP, test_exit, seed, 0, H, image_offset, ensemble=True,
                                                stop_on=stop_on, Q=Q, QH=QH)
    return tuple(a.cpu().numpy() for a in sums), t_used.cpu().numpy(), conv.cpu().numpy().astype(bool), act


def check_truncation(snap, got, t_used, which=(0, 1, 2, 3)):
    names = ("S", "H", "Q", "QH")
    for b in range(len(t_used)):
        ref = snap[int(t_used[b])]
        for i in which:
            g, r = (got[i][:, :, b], ref[i][:, :, b]) if got[i].ndim == 4 else (got[i][:, b], ref[i][:, b])
            np.testing.assert_array_equal(g, r, err_msg=f"{names[i]} of image {b} at t_used={int(t_used[b])}")


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("name", sorted(MODELS))
def test_stop_on_ensemble_equals_the_fixed_run_truncated_at_t_used(name, dt):
    seed = 11
    eng = engine(name, dt)
    x = synthetic_images(B, seed=21).to(DEV)
    snap = snapshots(eng, x, seed, key=(name, dt, seed))
    qs = q_sums(snap)
    e = eng.n_exits - 1
    for rule, q in RULES:
        thr = pick_threshold(qs, e, rule, q)
        got, t_used, conv, act = run(eng, x, thr, rule, seed, "ensemble")
        want_t, want_c, want_act = rederive(qs, e, rule, thr, B)
        print(f"{name}/{dt}/{rule}: threshold {thr:.6g}, active after steps {act}")
        np.testing.assert_array_equal(t_used, want_t)
        np.testing.assert_array_equal(conv, want_c)
        assert act == want_act
        assert len(set(t_used.tolist())) > 1, f"{rule}: images should retire at more than one step ({act})"
        check_truncation(snap, got, t_used)


@pytest.mark.parametrize("name", ["r18_block", "r18_exit_only_c100"])
def test_stop_on_exit_keeps_the_adaptive_bits_and_truncates_the_ensemble_sums(name):
    seed, dt = 11, "f16"
    eng = engine(name, dt)
    x = synthetic_images(B, seed=21).to(DEV)
    snap = snapshots(eng, x, seed, key=(name, dt, seed))
    e = eng.n_exits - 1
    for rule, q in RULES:
        thr = pick_threshold({t: (v[0],) for t, v in snap.items()}, e, rule, q)
        S0, H0 = eng.new_uncertainty_sums(B)
        t0, c0, act0 = eng.accumulate_adaptive(x, S0, T_MAX, thr, rule, T_STEP, -1, seed, 0, H0)
        got, t_used, conv, act = run(eng, x, thr, rule, seed, "exit")
        np.testing.assert_array_equal(t_used, t0.cpu().numpy())
        np.testing.assert_array_equal(conv, c0.cpu().numpy().astype(bool))
        assert act == act0 and len(set(t_used.tolist())) > 1
        np.testing.assert_array_equal(got[0], S0.cpu().numpy())
        np.testing.assert_array_equal(got[1], H0.cpu().numpy())
        check_truncation(snap, got, t_used)


def test_decisions_on_an_inner_ensemble_row():
    """test_exit = 1: the rule on the ensemble of exits 0..1 (row 1 of Q); every row is still truncated at the same t_used."""
    seed, name, dt = 11, "r18_block", "f16"
    eng = engine(name, dt)
    x = synthetic_images(B, seed=21).to(DEV)
    snap = snapshots(eng, x, seed, key=(name, dt, seed))
    qs = q_sums(snap)
    thr = pick_threshold(qs, 1, "sem", 0.5)
    got, t_used, conv, act = run(eng, x, thr, "sem", seed, "ensemble", test_exit=1)
    want_t, want_c, want_act = rederive(qs, 1, "sem", thr, B)
    np.testing.assert_array_equal(t_used, want_t)
    np.testing.assert_array_equal(conv, want_c)
    assert act == want_act
    check_truncation(snap, got, t_used)


def _check_readout_against_host(eng, x, r, seed, tau=None, what=""):
    """r: predict_adaptive(ensemble=True)'s dict; per image against decompose_ensemble_logits on forward_samples(x, t_used[b])."""
    t_used = r["t_used"].cpu().numpy()
    for t in sorted(set(t_used.tolist())):
        ref = decompose_ensemble_logits(eng.forward_samples(x, int(t), seed=seed).cpu().numpy(), tau)
        at = np.nonzero(t_used == t)[0]
        for dn, hn, tol in PAIRS:
            err = float(np.abs(r[dn].cpu().numpy()[:, at] - ref[hn][:, at]).max())
            assert err <= tol, f"{what} t_used={t} {dn}: {err:.3e} > {tol:.0e}"
    return t_used


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("name", ["r18_block", "r18_exit_only_c100"])
def test_finalize_per_image_against_the_host_restatement(name, dt):
    seed = 11
    eng = engine(name, dt)
    x = synthetic_images(B, seed=21).to(DEV)
    snap = snapshots(eng, x, seed, key=(name, dt, seed))
    thr = pick_threshold(q_sums(snap), eng.n_exits - 1, "sem", 0.4)
    r = eng.predict_adaptive(x, T_MAX, thr, t_step=T_STEP, seed=seed, ensemble=True, stop_on="ensemble")
    t_used = _check_readout_against_host(eng, x, r, seed, what=f"{name}/{dt}")
    assert len(set(t_used.tolist())) > 1
    assert tuple(r["Q"].shape) == (2, eng.n_exits, B, eng.out_dim) and tuple(r["QH"].shape) == (eng.n_exits, B)
    for k in ("pred_entropy", "exp_entropy", "mutual_info", "mean", "var", "logit_mean"):
        assert k in r
    # the sums are the snapshot's, the read-out is bmi_finalize_ensemble's at each image's own t
    check_truncation(snap, (None, None, r["Q"].cpu().numpy(), r["QH"].cpu().numpy()), t_used, which=(2, 3))
    for t in sorted(set(t_used.tolist())):
        Q, QH = (torch.from_numpy(snap[t][i]).to(DEV).contiguous() for i in (2, 3))
        ref = eng._finalize_ensemble_sums(Q, QH, t)
        idx = torch.from_numpy(np.nonzero(t_used == t)[0]).to(DEV)
        for k in ref:
            assert torch.equal(r[k][:, idx], ref[k][:, idx]), k
    again = eng.finalize_ensemble_per_image(r["Q"], r["QH"], r["t_used"])
    assert all(torch.equal(again[k], r[k]) for k in again)
    eng.check_finite()


def test_image_offset_share_equals_its_rows_of_the_whole_batch():
    Bw, off, n, seed = 48, 16, 16, 9
    eng = engine("r18_block", "f16", max_batch=Bw)
    assert eng.image_offset_ok(off)
    x = synthetic_images(Bw, seed=25).to(DEV)
    snap = snapshots(eng, x, seed)
    thr = pick_threshold(q_sums(snap), eng.n_exits - 1, "sem", 0.5)
    got, t_used, conv, _ = run(eng, x, thr, "sem", seed, "ensemble")
    assert len(set(t_used.tolist())) > 1
    part, tu, cv, _ = run(eng, x[off:off + n].contiguous(), thr, "sem", seed, "ensemble", image_offset=off)
    np.testing.assert_array_equal(tu, t_used[off:off + n])
    np.testing.assert_array_equal(cv, conv[off:off + n])
    for whole, share in zip(got, part):
        np.testing.assert_array_equal(share, whole[..., off:off + n, :] if whole.ndim == 4 else whole[..., off:off + n])


def test_temperature_members_are_the_tempered_distributions():
    seed = 7
    eng = engine("r18_block", "f16x2")
    x = synthetic_images(B, seed=26).to(DEV)
    tau = [0.6 + 0.45 * e for e in range(eng.n_exits)]
    plain = eng.predict_adaptive(x, T_MAX, -1.0, t_step=T_STEP, seed=seed, ensemble=True, stop_on="ensemble")
    eng.set_temperature(tau)
    try:
        snap = snapshots(eng, x, seed)
        qs = q_sums(snap)
        e = eng.n_exits - 1
        thr = pick_threshold(qs, e, "sem", 0.4)
        r = eng.predict_adaptive(x, T_MAX, thr, t_step=T_STEP, seed=seed, ensemble=True, stop_on="ensemble")
        t_used = _check_readout_against_host(eng, x, r, seed, tau, "tempered")
        want_t, want_c, want_act = rederive(qs, e, "sem", thr, B)
        np.testing.assert_array_equal(t_used, want_t)
        assert r["active_after_step"] == want_act and len(set(t_used.tolist())) > 1
        check_truncation(snap, (None, None, r["Q"].cpu().numpy(), r["QH"].cpu().numpy()), t_used, which=(2, 3))
        full = eng.predict_adaptive(x, T_MAX, -1.0, t_step=T_STEP, seed=seed, ensemble=True, stop_on="ensemble")
        assert (full["ens_mean"] - plain["ens_mean"]).abs().max().item() > 1e-3
    finally:
        eng.set_temperature(None)


def test_nobody_converges_equals_predict_ensemble():
    seed = 3
    eng = engine("r18_block", "f16")
    x = synthetic_images(B, seed=23).to(DEV)
    r = eng.predict_adaptive(x, T_MAX, -1.0, t_step=T_STEP, seed=seed, ensemble=True, stop_on="ensemble")
    assert (r["t_used"] == T_MAX).all() and not r["converged"].any() and r["active_after_step"] == [B, B, B]
    p = eng.predict_ensemble(x, T_MAX, seed=seed)
    for k in p:
        assert torch.equal(r[k], p[k]), k


def test_errors():
    x = synthetic_images(8, seed=27).to(DEV)
    exact = engine("r18_block", "f32", max_batch=8)
    with pytest.raises(_lib.BmiError) as ei:
        exact.predict_adaptive(x, 8, 0.01, t_step=4, ensemble=True, stop_on="ensemble")
    assert ei.value.code == -95                                   # BMI_ERR_UNSUPPORTED
    eng = engine("r18_block", "f16", max_batch=8)
    with pytest.raises(ValueError):
        eng.predict_adaptive(x, 8, 0.01, t_step=4, stop_on="ensemble")
    with pytest.raises(ValueError):
        eng.accumulate_adaptive(x, eng.new_moments(8), 8, 0.01, t_step=4, stop_on="ensemble")
    with pytest.raises(ValueError):
        eng.predict_adaptive(x, 8, 0.01, t_step=4, ensemble=True, stop_on="mean")
    # a scratch one byte short: BMI_ERR_NOMEM before any launch, every output still zero
    S, H, Q, QH = eng.new_ensemble_sums(8)
    need = int(eng.lib.bmi_ensemble_scratch_bytes(eng.handle, 8))
    scratch = torch.empty(need, dtype=torch.uint8, device=DEV)
    t_used = torch.zeros(8, dtype=torch.int32, device=DEV)
    conv = torch.zeros(8, dtype=torch.uint8, device=DEV)
    act = (C.c_int32 * 2)()

    def call(nbytes, stop_on=1, q1=Q[0].data_ptr()):
        return eng.lib.bmi_forward_mcd_adaptive_ensemble(
            eng.handle, x.data_ptr(), 8, 0, 8, 4, 7, 0, 0, 0.01, eng.n_exits - 1, stop_on, S[0].data_ptr(), S[1].data_ptr(), S[2].data_ptr(),
            H.data_ptr(), q1, Q[1].data_ptr(), QH.data_ptr(), scratch.data_ptr(), nbytes, t_used.data_ptr(), conv.data_ptr(), act,
            eng.workspace.data_ptr(), eng.workspace_bytes, C.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert call(need - 1) == -12
    assert call(need, stop_on=2) == -22 and call(need, q1=None) == -22
    torch.cuda.synchronize()
    assert not S._base.any() and not t_used.any() and not conv.any() and list(act) == [0, 0]
    assert call(need) == 0
    torch.cuda.synchronize()
    assert Q.any() and (t_used > 0).all()
