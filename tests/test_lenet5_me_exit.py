"""Staged early exit inside the fused multi-exit LeNet-5 (csrc/lenet5_me_exit.hip behind ``LeNet5Engine.predict_early_exit``): rows and
decisions against the full run (``accumulate``) bit for bit, and against the float64 forward of tests/test_lenet5_me.py.  The statistic is
restated in float64 numpy (a division, a sort, a subtraction).  The float64 reference alone, on these inputs (B = 8, T = 10), has a widest
gap between adjacent sorted statistics of 0.054 .. 0.35 over the three models and both rules, against the 4e-3 required below."""
import functools

import numpy as np
import pytest
import torch

from bayesnn_fpga_amd.models import extra as bx
from bayesnn_fpga_amd.synthetic import synthetic_images, synthetic_weights_
from tests.helpers import build_seeded
from tests.test_lenet5_me import SEED, forward64, mirror

pytestmark = pytest.mark.gpu
MACS0, MACS1 = 392000 + 40000 + 8000, 1960000 + 8000      # conv1 + ex1conv1 + ex1fc1 | conv2 + fc1, per image; + T * 100 * C per stage


def stat_of(mean0, rule):
    top = np.sort(mean0, axis=1)
    return top[:, -1] if rule == "confidence" else top[:, -1] - top[:, -2]


@functools.lru_cache(maxsize=None)
def full_run(B, T, dropout_exit=True, p=0.2, out_dim=10):
    """The engine, the images and ``accumulate``'s sums of samples 0 .. T-1 (the existing path: left unchanged by the tests)."""
    x = synthetic_images(B, 1234, channels=1, size=28).to("cuda:0")
    eng = mirror(dropout_exit, p, out_dim).to("cuda:0").eval().engine(x.device, max_batch=B)
    return eng, x, eng.accumulate(x, eng.new_moments(B), 0, T, SEED)


def check_against_full(eng, x, S_full, T, rule, thr):
    B = x.shape[0]
    want = np.where(stat_of(S_full[0, 0].cpu().numpy() / T, rule) > thr, 0, 1)
    S = eng.new_moments(B)
    got = eng.accumulate_early_exit(x, S, T, thr, SEED, rule).cpu().numpy()
    assert got.dtype == np.int32 and np.array_equal(got, want), (got, want)
    assert torch.equal(S[:, 0], S_full[:, 0])
    stay = torch.from_numpy(want == 1).to(S.device)
    assert torch.equal(S[:, 1, stay], S_full[:, 1, stay]) and not S[:, 1, ~stay].any()
    return want


# T = 1: three empty waves; 5, 10: ragged shares; 70: a second 64-sample round with a ragged tail; B = 3, 5, 8: first keep bytes 4 elements early
@pytest.mark.parametrize("rule", ["confidence", "margin"])
@pytest.mark.parametrize("B,T", [(1, 1), (3, 5), (8, 10), (5, 70)])
def test_rows_and_decisions_equal_the_full_run(B, T, rule):
    eng, x, S_full = full_run(B, T)
    s = np.sort(stat_of(S_full[0, 0].cpu().numpy() / T, rule))
    mid = (s[(B - 1) // 2] + s[min((B - 1) // 2 + 1, B - 1)]) / 2      # between the two middle statistics
    for thr, left in ((-1.0, B), (2.0, 0), (mid, None)):
        want = check_against_full(eng, x, S_full, T, rule, thr)
        assert left is None or int((want == 0).sum()) == left
    if B >= 3:
        assert 0 < int((want == 0).sum()) < B      # both branches ran


@pytest.mark.parametrize("rule", ["confidence", "margin"])
@pytest.mark.parametrize("dropout_exit,p", [(True, 0.2), (True, 0.25), (False, 0.2)])
def test_decisions_and_exit_taken_against_the_float64_reference(dropout_exit, p, rule):
    B, T = 8, 10
    _, mean, var = forward64(mirror(dropout_exit, p), synthetic_images(B, 1234, channels=1, size=28), T)
    stat = stat_of(mean[0], rule)
    s = np.sort(stat)
    i = int(np.argmax(np.diff(s)))
    assert s[i + 1] - s[i] >= 4e-3      # four times the 1e-3 tolerance on a mean: a margin is a difference of two means
    want = np.where(stat > (s[i] + s[i + 1]) / 2, 0, 1)
    eng, x, _ = full_run(B, T, dropout_exit, p)
    r = eng.predict_early_exit(x, T, (s[i] + s[i + 1]) / 2, seed=SEED, rule=rule)
    got = r["exit_layer"].cpu().numpy()
    assert np.array_equal(got, want) and r["active_after"] == [int(want.sum()), 0]
    idx = np.arange(B)
    for name, have, ref in (("best_preds", r["best_preds"], mean[want, idx]), ("var", r["var"][r["exit_layer"].long(), torch.arange(B, device=x.device)], var[want, idx])):
        print(f"{name}: max |error| {np.abs(have.cpu().numpy() - ref).max():.3e} (tolerance 1.0e-03)")
        np.testing.assert_allclose(have.cpu().numpy(), ref, rtol=0, atol=1e-3, err_msg=name)


# three classes: lanes 3..31 carry nothing; a NaN threshold: nobody leaves; all leave; none leave
@pytest.mark.parametrize("out_dim,thr", [(3, 0.4), (10, float("nan")), (10, -1.0), (10, 2.0)])
def test_edges_and_the_mac_model(out_dim, thr):
    B, T = 3, 5
    eng, x, S_full = full_run(B, T, out_dim=out_dim)
    want = check_against_full(eng, x, S_full, T, "confidence", thr)
    r = eng.predict_early_exit(x, T, thr, seed=SEED)
    stayed = int(want.sum())
    assert np.array_equal(r["exit_layer"].cpu().numpy(), want) and (thr == thr or stayed == B)
    assert r["macs_done"] == B * (MACS0 + T * 100 * out_dim) + stayed * (MACS1 + T * 100 * out_dim)
    assert r["macs_full"] == B * (MACS0 + MACS1 + 2 * T * 100 * out_dim) and (r["macs_done"] == r["macs_full"]) == (stayed == B)
    assert torch.equal(r["best_preds"], eng.finalize(S_full, T)["mean"][torch.from_numpy(want).to(x.device), torch.arange(B, device=x.device)])


def test_what_the_engine_refuses():
    eng, x, _ = full_run(3, 5)
    with pytest.raises(ValueError, match="rule"):
        eng.predict_early_exit(x, 5, 0.5, rule="entropy")
    single = synthetic_weights_(build_seeded(bx.LeNet5MC, dict(num_bayes_layer=1)), 0).to("cuda:0").eval().engine(x.device, max_batch=3)
    with pytest.raises(ValueError, match="multi-exit"):
        single.predict_early_exit(x, 5, 0.5)
