"""-m gpu: vote counts under staged early exit (bmi_forward_mcd_exit_staged_votes; MCDEngine.accumulate_early_exit with V,
predict_early_exit(ensemble_readout=True, votes=True)) against the same engine's full run ``predict_votes``: for every image the rows of
the exits it reached hold the full run's counts (the per-image exit count of csrc/votes_rows.hip cuts the running exit sum, it does not
change it), the rows behind them stay zero, and every other output is bmi_forward_mcd_exit_staged_ensemble's, bit for bit."""
import numpy as np
import pytest
import torch

from bayesnn_fpga_amd.models.resnet18.resnet18 import ResNet18MCEarlyExit
from bayesnn_fpga_amd.models.vgg19.vgg19 import VGG19MCEarlyExit
from bayesnn_fpga_amd.synthetic import synthetic_images, synthetic_weights_
from bayesnn_fpga_amd.train.uncertainty import vote_readout_numpy
from tests.helpers import build_seeded
from tests.test_staged_exit import _stat
from tests.test_staged_exit_ensemble import midpoint_near_median
from tests.test_votes_host import make_weights

pytestmark = [pytest.mark.gpu, pytest.mark.usefixtures("fp16_engine_default")]
DEV = "cuda:0"
B, T, SEED = 45, 4, 11
EXIT_ONLY = dict(dropout_exit=True, dropout=None, dropout_p=0.25, out_dim=10)
MODELS = {"r18_exit_only": (ResNet18MCEarlyExit, EXIT_ONLY), "vgg19": (VGG19MCEarlyExit, EXIT_ONLY)}

_ENGINES = {}


def engine(name):
    if name not in _ENGINES:
        cls, kw = MODELS[name]
        m = synthetic_weights_(build_seeded(cls, kw), 0)
        _ENGINES[name] = m.to(DEV).eval().engine(torch.device(DEV), max_batch=B, chunk_samples=T, dtype="f16")
    return _ENGINES[name]


def check(eng, x, first_exit, rule, ens_rule):
    full = eng.predict_votes(x, T, seed=SEED)
    Vf = torch.stack([full["votes"], full["ens_votes"]]).cpu().numpy()
    Sf, Hf, Qf, QHf = eng.new_ensemble_sums(B)
    eng.accumulate_ensemble(x, Sf, Hf, Qf, QHf, 0, T, SEED)
    thr = midpoint_near_median(_stat(Sf[0].cpu().numpy(), T, rule, ens_rule)[first_exit])
    r = eng.predict_early_exit(x, T, thr, seed=SEED, first_exit=first_exit, rule=rule, ensemble=ens_rule, ensemble_readout=True, votes=True)
    r0 = eng.predict_early_exit(x, T, thr, seed=SEED, first_exit=first_exit, rule=rule, ensemble=ens_rule, ensemble_readout=True)
    xl = r["exit_layer"].cpu().numpy()
    print(f"first_exit={first_exit}/{rule}/ensemble={ens_rule}: threshold {thr:.6g}, active after {r['active_after']}")
    assert len(set(xl.tolist())) >= 2, "at least two different exits should be taken"
    # exit_layer and the sums' read-outs are the staged ensemble call's
    for k, v in r0.items():
        if isinstance(v, torch.Tensor):
            assert torch.equal(r[k], v), k
        elif isinstance(v, dict):
            assert all(torch.equal(r[k][n], v[n]) for n in v), k
        else:
            assert r[k] == v, k
    # the sums themselves too
    S, H, Q, QH = eng.new_ensemble_sums(B)
    S0, H0, Q0, QH0 = eng.new_ensemble_sums(B)
    V = eng.new_vote_counts(B)
    a = eng.accumulate_early_exit(x, S, T, thr, seed=SEED, first_exit=first_exit, rule=rule, ensemble=ens_rule, H=H, Q=Q, QH=QH, V=V)
    a0 = eng.accumulate_early_exit(x, S0, T, thr, seed=SEED, first_exit=first_exit, rule=rule, ensemble=ens_rule, H=H0, Q=Q0, QH=QH0)
    assert torch.equal(a[0], a0[0]) and a[1] == a0[1]
    assert torch.equal(S, S0) and torch.equal(H, H0) and torch.equal(Q, Q0) and torch.equal(QH, QH0)
    assert torch.equal(V, r["V"])
    # the counts: the full run's on the rows an image reached, zero behind them
    Vn = r["V"].cpu().numpy()
    for e in range(eng.n_exits):
        reached = xl >= e
        np.testing.assert_array_equal(Vn[:, e][:, reached], Vf[:, e][:, reached], err_msg=f"V rows of exit {e}")
        assert not Vn[:, e][:, ~reached].any(), f"rows of exit {e} nobody reached must stay zero"
        assert (Vn[:, e][:, reached].sum(-1) == T).all()
    want = vote_readout_numpy(Vn)
    for pre, kind in (("", 0), ("ens_", 1)):
        assert np.array_equal(r[pre + "vote_class"].cpu().numpy(), want["vote_class"][kind])
        assert np.array_equal(r[pre + "variation_ratio"].cpu().numpy(), want["variation_ratio"][kind])
        assert torch.equal(r[pre + "votes"], r["V"][kind])
    return xl


@pytest.mark.parametrize("first_exit", [0, 1])
@pytest.mark.parametrize("name", sorted(MODELS))
def test_reached_rows_hold_the_full_runs_counts(name, first_exit):
    eng = engine(name)
    x = synthetic_images(B, seed=21).to(DEV)
    check(eng, x, first_exit, "confidence", False)
    check(eng, x, first_exit, "margin", True)
    eng.check_finite()


def test_weights_and_a_temperature():
    """The engine's calibration reaches the rows launch: the counts are still predict_votes' (which reads the same map and weights)."""
    eng = engine("r18_exit_only")
    x = synthetic_images(B, seed=22).to(DEV)
    plain = eng.predict_votes(x, T, seed=SEED)
    eng.set_ensemble_weights(make_weights(eng.n_exits, 3))
    eng.set_temperature([0.6 + 0.45 * e for e in range(eng.n_exits)])
    try:
        check(eng, x, 1, "confidence", True)
        cal = eng.predict_votes(x, T, seed=SEED)
        assert not torch.equal(cal["ens_votes"], plain["ens_votes"])       # the weights move votes: the comparison is not vacuous
    finally:
        eng.set_temperature(None)
        eng.set_ensemble_weights(None)


def test_everybody_leaves_at_the_first_tested_exit():
    eng = engine("r18_exit_only")
    x = synthetic_images(B, seed=21).to(DEV)
    full = eng.predict_votes(x, T, seed=SEED)
    r = eng.predict_early_exit(x, T, -1.0, seed=SEED, first_exit=1, ensemble_readout=True, votes=True)
    assert (r["exit_layer"] == 1).all()
    assert torch.equal(r["V"][:, :2], torch.stack([full["votes"], full["ens_votes"]])[:, :2]) and not r["V"][:, 2:].any()
    assert (r["vote_class"][2:] == -1).all() and (r["vote_class"][:2] >= 0).all()
