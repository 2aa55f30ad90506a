"""The host restatement of the exit-ensemble read-out (train/uncertainty.py: decompose_ensemble_logits) — pinned to the reference's own
ensemble output on the goldens' per-pass logits, to decompose_logits on row 0, to an independent torch-float64 computation, and shown
not to be derivable from the per-exit moments."""
import numpy as np
import pytest
import torch

from bayesnn_fpga_amd.train.uncertainty import decompose_ensemble_logits, decompose_logits
from tests.helpers import load_golden

WITH_REF_ENSEMBLE = ["resnet18_block_exit", "resnet18_exit_only", "resnet18_layer_exit", "resnet18_mask4_block_exit", "resnet18_mask8_exit_c100"]
CONFIGS = WITH_REF_ENSEMBLE + ["vgg19_exit_mc"]
ENTROPIES = ("pred_entropy", "exp_entropy", "mutual_info")


def _logits(name):
    return np.asarray(load_golden(f"{name}.npz")["logits"])


@pytest.mark.parametrize("name", WITH_REF_ENSEMBLE)
def test_mean_is_the_references_ensemble_output(name):
    """The reference's ensemble_output_sm (results_analyzer.py:260-269, fp32 softmax) to 1e-6."""
    g = load_golden(f"{name}.npz")
    r = decompose_ensemble_logits(g["logits"])
    err = float(np.abs(r["mean"] - g["go_ensemble_output_sm"]).max())
    print(f"{name}: max |mean - go_ensemble_output_sm| = {err:.3e}")
    np.testing.assert_allclose(r["mean"], g["go_ensemble_output_sm"], rtol=0, atol=1e-6)


def _torch_restatement(logits):
    """Written differently on purpose: log_softmax().exp(), cumsum over the exits, var(unbiased=False), xlogy."""
    l = torch.from_numpy(np.asarray(logits, dtype=np.float32)).double()
    E = l.shape[1]
    p = torch.log_softmax(l, dim=-1).exp()
    q = p.cumsum(dim=1) / torch.arange(1, E + 1, dtype=torch.float64).view(1, E, 1, 1)
    mean = q.mean(dim=0)
    var = q.var(dim=0, unbiased=False)
    pred = -torch.xlogy(mean, mean).sum(-1)
    exp = (-torch.xlogy(q, q).sum(-1)).mean(dim=0)
    return dict(mean=mean.numpy(), var=var.numpy(), pred_entropy=pred.numpy(), exp_entropy=exp.numpy(),
                mutual_info=(pred - exp).clamp_min(0).numpy())


@pytest.mark.parametrize("name", CONFIGS)
def test_row_zero_is_exit_zero_and_an_independent_computation_agrees(name):
    logits = _logits(name)
    r = decompose_ensemble_logits(logits)
    d0 = decompose_logits(logits[:, 0])
    np.testing.assert_allclose(r["mean"][0], d0["mean"], rtol=0, atol=1e-15)
    for q in ENTROPIES:
        np.testing.assert_allclose(r[q][0], d0[q], rtol=0, atol=1e-12)
    t = _torch_restatement(logits)
    for q in ("mean", "var") + ENTROPIES:
        assert r[q].shape == t[q].shape
        np.testing.assert_allclose(r[q], t[q], rtol=0, atol=1e-12, err_msg=q)


def test_the_variance_is_not_that_of_independent_exits():
    """The exits of one pass are correlated: on resnet18_exit_only the ensemble variance is more than 1e-3 (the project's bar) away from
    sum_i var_i / (e + 1)^2, what the per-exit moments alone would give."""
    logits = _logits("resnet18_exit_only")
    r = decompose_ensemble_logits(logits)
    z = logits.astype(np.float64)
    z = z - z.max(-1, keepdims=True)
    p = np.exp(z) / np.exp(z).sum(-1, keepdims=True)
    var_i = p.var(axis=0)                                      # [E, B, C]
    E = var_i.shape[0]
    indep = np.cumsum(var_i, axis=0) / (np.arange(1, E + 1).reshape(E, 1, 1) ** 2)
    gap = float(np.abs(r["var"] - indep).max())
    print(f"max |ens_var - independent| = {gap:.3e}")
    assert gap > 1e-3
    np.testing.assert_allclose(r["var"][0], indep[0], rtol=0, atol=1e-15)     # (one exit: nothing to correlate with)


@pytest.mark.parametrize("name", CONFIGS)
def test_the_ensembles_carry_mutual_information(name):
    r = decompose_ensemble_logits(_logits(name))
    print(f"{name}: min ens_mutual_info = {r['mutual_info'].min():.3e}")
    assert (r["mutual_info"] > 1e-4).all()
    assert (r["var"] >= 0).all() and (r["exp_entropy"] >= 0).all()


@pytest.mark.parametrize("name", ["resnet18_block_exit", "vgg19_exit_mc"])
def test_temperature(name):
    logits = _logits(name)
    E = logits.shape[1]
    r = decompose_ensemble_logits(logits)
    ones = decompose_ensemble_logits(logits, tau=np.ones(E))
    for q in r:
        assert np.array_equal(r[q], ones[q]), q
    tau = np.linspace(0.6, 2.3, E)
    inv = (1.0 / tau.astype(np.float32).astype(np.float64)).astype(np.float32)
    z = (logits.astype(np.float32) * inv[None, :, None, None]).astype(np.float32).astype(np.float64)
    rt = decompose_ensemble_logits(logits, tau=tau)
    want = decompose_ensemble_logits(z)                   # float64(float32(l) * float32(1 / tau)) as plain logits
    for q in rt:
        assert np.array_equal(rt[q], want[q]), q
    assert np.abs(rt["mean"] - r["mean"]).max() > 1e-3
    scalar = decompose_ensemble_logits(logits, tau=1.7)
    full = decompose_ensemble_logits(logits, tau=[1.7] * E)
    assert all(np.array_equal(scalar[q], full[q]) for q in full)
    with pytest.raises(ValueError):
        decompose_ensemble_logits(logits, tau=[1.0] * (E + 1))


def test_peaky_logits_stay_finite():
    """Normal logits x 100 at C = 100: most probabilities underflow; everything finite, entropies >= 0."""
    rng = np.random.default_rng(5)
    logits = (rng.standard_normal((7, 4, 6, 100)) * 100).astype(np.float32)
    assert np.abs(logits).max() > 300
    r = decompose_ensemble_logits(logits)
    for q in r:
        assert np.isfinite(r[q]).all(), q
    assert all((r[q] >= 0).all() for q in ENTROPIES) and (r["var"] >= 0).all()
    np.testing.assert_allclose(r["mean"].sum(-1), 1.0, rtol=0, atol=1e-12)
