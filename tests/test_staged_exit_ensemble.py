"""-m gpu: the exit-ensemble read-out under staged early exit (bmi_forward_mcd_exit_staged_ensemble; MCDEngine.accumulate_early_exit with
Q / QH, predict_early_exit(ensemble_readout=True)) against the same engine's full run ``accumulate_ensemble(0, T)``: for every image the
rows of the exits it reached are the full run's bit for bit (the per-image exit count of csrc/ensemble.hip cuts the running exit sum, it
does not change it), the rows of the exits it never reached stay zero, and S / H / exit_layer are the staged call's without the read-out."""
import ctypes as C

import numpy as np
import pytest
import torch

from bayesnn_fpga_amd import _lib
from bayesnn_fpga_amd.models.resnet18.resnet18 import ResNet18MCEarlyExit
from bayesnn_fpga_amd.synthetic import synthetic_images, synthetic_weights_
from tests.helpers import build_seeded
from tests.test_staged_exit import _stat

pytestmark = [pytest.mark.gpu, pytest.mark.usefixtures("fp16_engine_default")]
DEV = "cuda:0"
B, T = 45, 8

MODELS = {
    "r18_exit_only_c10": (ResNet18MCEarlyExit, dict(dropout_exit=True, dropout=None, dropout_p=0.25, out_dim=10)),
    "r18_exit_only_c100": (ResNet18MCEarlyExit, dict(dropout_exit=True, dropout=None, dropout_p=0.25, out_dim=100)),
    "r18_block": (ResNet18MCEarlyExit, dict(dropout_exit=True, dropout="block", dropout_p=0.25, out_dim=10)),
}
RULES = [("confidence", False), ("margin", False), ("confidence", True), ("margin", True)]

_ENGINES = {}
_FULL = {}


def engine(name, dt):
    if (name, dt) not in _ENGINES:
        cls, kw = MODELS[name]
        m = synthetic_weights_(build_seeded(cls, kw), 0)
        _ENGINES[name, dt] = m.to(DEV).eval().engine(torch.device(DEV), max_batch=B, chunk_samples=T, dtype=dt)
    return _ENGINES[name, dt]


def full_run(name, dt, seed):
    """(engine, x, (S, H, Q, QH) of accumulate_ensemble(0, T) on the host): once per (model, dtype)."""
    eng = engine(name, dt)
    x = synthetic_images(B, seed=21).to(DEV)
    if (name, dt, seed) not in _FULL:
        sums = eng.new_ensemble_sums(B)
        eng.accumulate_ensemble(x, *sums, 0, T, seed)
        _FULL[name, dt, seed] = tuple(a.cpu().numpy().copy() for a in sums)
    return eng, x, _FULL[name, dt, seed]


def midpoint_near_median(values):
    """A midpoint between two neighbouring observed statistics, more than 1e-8 apart, nearest their median: no image sits on it."""
    v = np.unique(values[np.isfinite(values)])
    mids = [(a + b) / 2 for a, b in zip(v[:-1], v[1:]) if b - a > 1e-8]
    return float(min(mids, key=lambda m: abs(m - np.median(values))))


def staged(eng, x, thr, seed, first_exit, rule, ens_rule):
    sums = eng.new_ensemble_sums(B)
    S, H, Q, QH = sums
    xl, act = eng.accumulate_early_exit(x, S, T, thr, seed=seed, first_exit=first_exit, rule=rule, ensemble=ens_rule, H=H, Q=Q, QH=QH)
    return tuple(a.cpu().numpy() for a in sums), xl.cpu().numpy(), act


def check_rows(eng, got, xl, full):
    _, _, Q, QH = got
    _, _, Qf, QHf = full
    for e in range(eng.n_exits):
        reached = xl >= e
        np.testing.assert_array_equal(Q[:, e][:, reached], Qf[:, e][:, reached], err_msg=f"Q rows of exit {e}")
        np.testing.assert_array_equal(QH[e][reached], QHf[e][reached], err_msg=f"QH rows of exit {e}")
        assert not Q[:, e][:, ~reached].any() and not QH[e][~reached].any(), f"rows of exit {e} nobody reached must stay zero"


@pytest.mark.parametrize("first_exit", [0, 1])
@pytest.mark.parametrize("dt", ["f16", "f16x2"])
@pytest.mark.parametrize("name", sorted(MODELS))
def test_reached_rows_are_the_full_runs_and_the_others_stay_zero(name, dt, first_exit):
    seed = 11
    eng, x, full = full_run(name, dt, seed)
    for rule, ens_rule in RULES:
        thr = midpoint_near_median(_stat(full[0][0], T, rule, ens_rule)[first_exit])
        got, xl, act = staged(eng, x, thr, seed, first_exit, rule, ens_rule)
        print(f"{name}/{dt}/first_exit={first_exit}/{rule}/ensemble={ens_rule}: threshold {thr:.6g}, active after {act}")
        assert len(set(xl.tolist())) >= 2, f"at least two different exits should be taken ({act})"
        check_rows(eng, got, xl, full)
        S0, H0 = eng.new_uncertainty_sums(B)
        xl0, act0 = eng.accumulate_early_exit(x, S0, T, thr, seed=seed, first_exit=first_exit, rule=rule, ensemble=ens_rule, H=H0)
        np.testing.assert_array_equal(xl, xl0.cpu().numpy())
        assert act == act0
        np.testing.assert_array_equal(got[0], S0.cpu().numpy())
        np.testing.assert_array_equal(got[1], H0.cpu().numpy())


@pytest.mark.parametrize("first_exit", [0, 1])
@pytest.mark.parametrize("name", ["r18_exit_only_c100", "r18_block"])
def test_everybody_leaves_at_the_first_tested_exit(name, first_exit):
    """A threshold below every statistic: the call returns early, behind the first decision — the reached rows are filled all the same."""
    seed, dt = 11, "f16"
    eng, x, full = full_run(name, dt, seed)
    got, xl, act = staged(eng, x, -1.0, seed, first_exit, "confidence", False)
    assert (xl == first_exit).all() and act[first_exit] == 0 and act[-1] == 0
    check_rows(eng, got, xl, full)
    assert got[2][:, :first_exit + 1].all(), "the reached rows hold T samples of probabilities"


def test_nobody_leaves_equals_accumulate_ensemble():
    seed, name, dt = 11, "r18_block", "f16"
    eng, x, full = full_run(name, dt, seed)
    got, xl, act = staged(eng, x, 2.0, seed, 1, "confidence", False)
    assert (xl == eng.n_exits - 1).all() and act[-1] == B
    for g, f in zip(got, full):
        np.testing.assert_array_equal(g, f)


def test_predict_early_exit_readout():
    seed, name, dt = 11, "r18_exit_only_c100", "f16"
    eng, x, full = full_run(name, dt, seed)
    ref = eng.predict_ensemble(x, T, seed=seed)
    thr = midpoint_near_median(_stat(full[0][0], T, "confidence", True)[1])
    r = eng.predict_early_exit(x, T, thr, seed=seed, ensemble=True, ensemble_readout=True)
    plain = eng.predict_early_exit(x, T, thr, seed=seed, ensemble=True, uncertainty=True)
    xl = r["exit_layer"]
    assert torch.equal(xl, plain["exit_layer"]) and r["active_after"] == plain["active_after"] and len(set(xl.tolist())) >= 2
    for k in plain:
        if isinstance(plain[k], torch.Tensor):
            assert torch.equal(r[k], plain[k]), k
        else:
            assert r[k] == plain[k], k
    idx = torch.arange(B, device=DEV)
    for e in range(eng.n_exits):
        reached = xl >= e
        for k in ("ens_mean", "ens_var", "ens_pred_entropy", "ens_exp_entropy", "ens_mutual_info"):
            assert torch.equal(r[k][e][reached], ref[k][e][reached]), (k, e)
    assert set(r["best_ens"]) == {"mean", "var", "pred_entropy", "exp_entropy", "mutual_info"}
    for k, v in r["best_ens"].items():
        assert torch.equal(v, ref["ens_" + k][xl.long(), idx]), k
    # the ensemble mean of per-sample ensembles is the ensemble of the means (best_preds) up to the order of summation
    np.testing.assert_allclose(r["best_ens"]["mean"].cpu().numpy(), r["best_preds"].cpu().numpy(), rtol=0, atol=1e-6)
    eng.check_finite()


def test_errors():
    eng = engine("r18_exit_only_c10", "f16")
    x = synthetic_images(B, seed=21).to(DEV)
    S, H, Q, QH = eng.new_ensemble_sums(B)
    with pytest.raises(ValueError):
        eng.accumulate_early_exit(x, S, T, 0.5, H=H, Q=Q)                 # Q without QH
    with pytest.raises(ValueError):
        eng.accumulate_early_exit(x, S, T, 0.5, Q=Q, QH=QH)               # the read-out needs H as well
    need = int(eng.lib.bmi_ensemble_scratch_bytes(eng.handle, B))
    scratch = torch.empty(need, dtype=torch.uint8, device=DEV)
    xl = torch.zeros(B, dtype=torch.int32, device=DEV)
    act = (C.c_int32 * eng.n_exits)()
    rule = _lib.ExitRule(0, 0, 0.5, 1)

    def call(nbytes, qh=QH.data_ptr()):
        return eng.lib.bmi_forward_mcd_exit_staged_ensemble(
            eng.handle, x.data_ptr(), B, T, 7, 0, C.byref(rule), S[0].data_ptr(), S[1].data_ptr(), S[2].data_ptr(), H.data_ptr(),
            Q[0].data_ptr(), Q[1].data_ptr(), qh, scratch.data_ptr(), nbytes, xl.data_ptr(), act, eng.workspace.data_ptr(),
            eng.workspace_bytes, C.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert call(need - 1) == -12 and call(need, qh=None) == -22
    torch.cuda.synchronize()
    assert not S._base.any() and not xl.any() and list(act) == [0] * eng.n_exits
    assert call(need) == 0
