"""-m gpu: the joint temperature fit of the exit ensembles — the on-device objective (bmi_nll_ensemble_temperature_grid) against its numpy
restatement on host-made logits over every path of the launcher (several images per workgroup, one image, sample chunks; candidate
slices; every kind of mask), its error codes, and EnsembleTemperatureScaling end to end against coordinate_search run on the host."""
import itertools

import numpy as np
import pytest
import torch

from bayesnn_fpga_amd import _lib
from bayesnn_fpga_amd.models.resnet18.resnet18 import ResNet18MCEarlyExit
from bayesnn_fpga_amd.synthetic import synthetic_images, synthetic_weights_
from bayesnn_fpga_amd.train import EnsembleTemperatureScaling
from bayesnn_fpga_amd.train.calibration import coordinate_search, ensemble_nll_grid_numpy, temper_logits
from tests.helpers import build_seeded

pytestmark = [pytest.mark.gpu, pytest.mark.usefixtures("fp16_engine_default")]
DEV = "cuda:0"
HEADS = ("ex1linear", "ex2linear", "ex3linear", "linear")
EXIT_ONLY_10 = dict(dropout_exit=True, dropout=None, dropout_p=0.25, out_dim=10)
TAUS = [0.05, 0.7, 1.0, 2.5, 20.0]


def _model(kw, gain=None):
    m = synthetic_weights_(build_seeded(ResNet18MCEarlyExit, kw), 0)
    if gain:                     # the "trained-like" twin: every classifier x 24
        with torch.no_grad():
            for n in HEADS:
                getattr(m, n).weight.mul_(gain)
    return m.to(DEV).eval()


@pytest.fixture(scope="module")
def eng():
    """An engine to call through: the objective reads the caller's logits, not the model."""
    return _model(EXIT_ONLY_10).engine(torch.device(DEV), max_batch=2, dtype="f16")


def _host_logits(T, E, B, Cn, scale, seed):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(T, E, B, Cn, generator=g) * (scale / 3)).clamp_(-scale, scale)


def _cand(G):
    return np.array([0.05], np.float32) if G == 1 else np.exp(np.linspace(np.log(0.05), np.log(20.0), G)).astype(np.float32)


def _chunked(T, E, Cn):
    """Whether the launcher runs this shape in sample chunks: T * E rows beyond what one staged chunk holds (include/bayesnn_fpga_amd.h)."""
    return T * E > min(_lib.NLL_ENS_ROWS, _lib.NLL_ENS_SLAB // (Cn | 1))


# ---- 6. the kernel against its restatement ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("E", [1, 4, 5])
@pytest.mark.parametrize("Cn", [10, 100])
def test_ensemble_nll_grid_equals_its_numpy_restatement(eng, Cn, E):
    """ensemble_nll_grid against ensemble_nll_grid_numpy on torch.randn logits scaled to +-3 and +-300, to 1e-9 relative — the bound
    tests/test_temperature.py holds bmi_nll_temperature_grid to, for its reason: each image's term carries a few ulp of float64 from
    exp / log, summing a few dozen of them stays far below 1e-11, and 1e-9 leaves two orders of margin for the device's libm.
    T in {1, 10, 30} x B in {7, 37} (ragged against every image run) x mask in {none, {0}, {E-1}, all}, G in {1, 5, 33} and the two
    scales rotating over them; tau and the candidates down to 0.05.  T = 30 at E = 4, C = 100 is the sample-chunked path, by the
    launcher's own limits.  Every value finite, two identical calls torch.equal, the rows below a single varied exit the same bits for
    every candidate, row 0 under mask {0} = nll_grid's row 0."""
    assert _chunked(30, 4, 100) and not _chunked(10, 4, 100) and not _chunked(10, 5, 100)
    full = {s: _host_logits(30, E, 37, Cn, s, seed=Cn + E).to(DEV) for s in (3.0, 300.0)}
    rng = np.random.default_rng(Cn * 7 + E)
    labels_all = rng.integers(0, Cn, 37)
    tau = TAUS[:E]
    masks = [None, [0], [E - 1], list(range(E))]
    worst, paths = 0.0, set()
    for k, (T, B, vary) in enumerate(itertools.product((1, 10, 30), (7, 37), masks)):
        G, scale = (1, 5, 33)[k % 3], (3.0, 300.0)[(k // 3) % 2]
        paths.add(_chunked(T, E, Cn))
        logits = full[scale][:T, :, :B].contiguous()
        y = torch.from_numpy(labels_all[:B])
        cand = _cand(G)
        got = eng.ensemble_nll_grid(logits, y, tau, vary, cand)
        assert torch.equal(got, eng.ensemble_nll_grid(logits, y, tau, vary, cand))
        assert got.shape == (E, G) and got.dtype == torch.float64
        if vary is not None and len(vary) == 1 and vary[0] > 0:
            assert torch.equal(got[:vary[0]], got[:vary[0], :1].expand(-1, G)), (T, B, G, vary)
        if vary == [0]:
            per_exit = eng.nll_grid(logits, y, np.stack([cand] * E))
            np.testing.assert_allclose(got[0].cpu().numpy(), per_exit[0].cpu().numpy(), rtol=1e-12, atol=0)
        got = got.cpu().numpy()
        ref = ensemble_nll_grid_numpy(logits.cpu().numpy(), labels_all[:B], tau, vary, cand)
        assert np.isfinite(got).all() and np.isfinite(ref).all()
        err = float(np.abs(got / ref - 1).max())
        worst = max(worst, err)
        assert err <= 1e-9, (T, B, G, vary, scale, err)
    print(f"C {Cn} E {E}: worst relative difference to numpy {worst:.2e}; chunked path taken: {sorted(paths)}")
    if (Cn, E) == (100, 4):
        assert paths == {False, True}


def test_accumulation_over_batches_and_more_than_64_images(eng):
    """Two batches (B = 20 and 17) accumulated into one ``out`` = numpy on the concatenation to 1e-12; B = 130 covers the stride of the
    fixed-order sum over images (64 lanes)."""
    E, Cn, T = 4, 10, 10
    full = _host_logits(T, E, 130, Cn, 30.0, seed=5).to(DEV)
    labels = np.random.default_rng(5).integers(0, Cn, 130)
    cand, tau = _cand(33), TAUS[:E]
    for vary in (2, range(E)):
        a, b = full[:, :, :20].contiguous(), full[:, :, 20:37].contiguous()
        out = eng.ensemble_nll_grid(a, torch.from_numpy(labels[:20]), tau, vary, cand)
        out = eng.ensemble_nll_grid(b, torch.from_numpy(labels[20:37]), tau, vary, cand, out=out).cpu().numpy()
        ref = ensemble_nll_grid_numpy(full[:, :, :37].cpu().numpy(), labels[:37], tau, vary, cand)
        np.testing.assert_allclose(out, ref, rtol=1e-12, atol=0)
        got = eng.ensemble_nll_grid(full, torch.from_numpy(labels), tau, vary, cand).cpu().numpy()
        ref = ensemble_nll_grid_numpy(full.cpu().numpy(), labels, tau, vary, cand)
        err = float(np.abs(got / ref - 1).max())
        print(f"B = 130, vary {vary}: relative difference to numpy {err:.2e}")
        assert err <= 1e-9


def test_python_checks(eng):
    logits = _host_logits(2, 4, 3, 10, 3.0, seed=1).to(DEV)
    y = torch.zeros(3, dtype=torch.int64)
    for bad in (dict(vary=4), dict(vary=[0, -1]), dict(tau=[1.0, 1.0]), dict(tau=[1.0, 0.0, 1.0, 1.0]), dict(cand=np.ones((2, 2))),
                dict(out=torch.zeros(4, 2, dtype=torch.float64, device=DEV))):
        kw = dict(tau=1.0, vary=None, cand=[1.0])
        kw.update(bad)
        with pytest.raises(ValueError):
            eng.ensemble_nll_grid(logits, y, **kw)
    with pytest.raises(ValueError):
        eng.ensemble_nll_grid(logits.double(), y, 1.0, None, [1.0])
    none = eng.ensemble_nll_grid(logits, y, None, None, [1.0])
    assert torch.equal(none, eng.ensemble_nll_grid(logits, y, [1.0] * 4, None, [7.0]))       # no exit varies: the candidate's value is not read


# ---- 7. errors on the device --------------------------------------------------------------------------------------------------------
def test_errors_write_nothing(eng):
    """A scratch one byte short: BMI_ERR_NOMEM; E = 33 and a row that does not fit the staging buffer: BMI_ERR_UNSUPPORTED; ``out`` keeps
    its sentinel."""
    lib = eng.lib
    NOMEM, UNSUPPORTED = -12, -95                       # BMI_ERR_NOMEM, BMI_ERR_UNSUPPORTED of include/bayesnn_fpga_amd.h
    T, B, G = 2, 3, 2

    def call(E, Cn, short=0):
        logits = torch.zeros(T, E, B, Cn, device=DEV)
        y = torch.zeros(B, dtype=torch.int32, device=DEV)
        tau, cand = torch.ones(E, device=DEV), torch.ones(G, device=DEV)
        out = torch.full((E, G), -7.5, dtype=torch.float64, device=DEV)
        need = lib.bmi_nll_ensemble_temperature_scratch_bytes(E, B, G)
        assert need == E * G * B * 8
        scratch = torch.zeros(need, dtype=torch.uint8, device=DEV)
        with torch.cuda.device(DEV):
            rc = lib.bmi_nll_ensemble_temperature_grid(logits.data_ptr(), T, E, B, Cn, y.data_ptr(), tau.data_ptr(), 0, cand.data_ptr(), G,
                                                       out.data_ptr(), scratch.data_ptr(), need - short, None)
        torch.cuda.synchronize()
        return rc, out
    rc, out = call(4, 10)
    assert rc == _lib.BMI_OK and not bool((out == -7.5).any())
    for args, want in (((4, 10, 1), NOMEM), ((33, 10), UNSUPPORTED), ((4, _lib.NLL_ENS_SLAB // 4 + 1), UNSUPPORTED)):
        rc, out = call(*args)               # (the last one: E * (C | 1) floats beyond the staging buffer)
        assert rc == want, (args, rc)
        assert bool((out == -7.5).all()), args
    with pytest.raises(_lib.BmiError):
        eng.ensemble_nll_grid(torch.zeros(1, 33, 2, 4, device=DEV), torch.zeros(2, dtype=torch.int64), 1.0, None, [1.0])


# ---- 8. the fit, end to end ---------------------------------------------------------------------------------------------------------
FIT_SIZES = [400, 200]
FIT_T, FIT_SEED = 10, 5


def _ensemble_nll_of_mean(mean, labels):
    return float(-np.log(mean[np.arange(len(labels)), labels]).sum())


def test_ensemble_temperature_scaling_fit_end_to_end(tmp_path, monkeypatch):
    """EnsembleTemperatureScaling.fit over a two-batch loader (400 + 200) of the x24 twin (exit-only dropout, C = 10, f16x2, T = 10) with
    teacher labels drawn from the LAST ENSEMBLE ROW's predictive at tau* = 3 (temper_logits of the engine's own raw logits).  The trace
    never increases, the joint fit is no worse than the per-exit fit and better than tau = 1 on the ensemble's NLL, the result is the
    restatement's value at the fitted vector to 1e-9, and the final objective agrees with coordinate_search run on the host over the
    restatement from the same init within 10 sweep_rtol: two runs whose objectives differ by 1e-9 may stop one sweep apart, and a last
    sweep moves the objective by at most about sweep_rtol (the temperatures are not compared: flat directions are legitimate)."""
    Cn, N, E = 10, sum(FIT_SIZES), 4
    m = _model(EXIT_ONLY_10, gain=24.0)
    m.engine_dtype = "f16x2"
    x = synthetic_images(N, seed=31)
    offs = np.concatenate([[0], np.cumsum(FIT_SIZES)])
    eng = m.engine(torch.device(DEV), max_batch=max(FIT_SIZES))
    raw = np.concatenate([eng.forward_samples(x[offs[k]:offs[k + 1]].to(DEV), FIT_T, seed=FIT_SEED + k).cpu().numpy()
                          for k in range(len(FIT_SIZES))], axis=2)
    mean, _ = temper_logits(raw, 3.0)
    q = mean.mean(0)                                    # the last ensemble row: the mean of all E exits' T-means
    rng = np.random.default_rng(7)
    labels = np.array([rng.choice(Cn, p=p / p.sum()) for p in q])
    y = torch.from_numpy(labels)
    loader = [(x[offs[k]:offs[k + 1]], y[offs[k]:offs[k + 1]]) for k in range(len(FIT_SIZES))]

    def last_row_nll():
        e = m.engine(torch.device(DEV), max_batch=max(FIT_SIZES))
        rows = [e.predict_ensemble(x[offs[k]:offs[k + 1]].to(DEV), FIT_T, seed=FIT_SEED + k)["ens_mean"][-1].cpu().numpy()
                for k in range(len(FIT_SIZES))]
        return _ensemble_nll_of_mean(np.concatenate(rows), labels)
    before = last_row_nll()

    ets = EnsembleTemperatureScaling(m, loader, gpu=0, mc_passes=FIT_T, seed=FIT_SEED)
    r = ets.fit()
    print(f"fit: tau {r['tau']}, sweeps {r['sweeps']}, trace {r['trace']}\n  ones {r['nll_ones']}\n  per-exit {r['nll_per_exit']}\n  init {r['nll_init']}"
          f"\n  after {r['nll_after']}")
    assert r["n"] == N
    assert np.all(np.diff(r["trace"]) <= 0) and r["trace"][0] <= r["nll_init"][-1]
    assert r["nll_after"][-1] <= r["nll_per_exit"][-1]
    assert r["nll_after"][-1] < r["nll_ones"][-1]
    np.testing.assert_allclose(r["nll_per_exit"], r["nll_init"], rtol=1e-12)
    np.testing.assert_allclose(ensemble_nll_grid_numpy(raw, labels, r["tau"], None, [1.0])[:, 0], r["nll_after"], rtol=1e-9, atol=0)
    np.testing.assert_allclose(ensemble_nll_grid_numpy(raw, labels, 1.0, None, [1.0])[:, 0], r["nll_ones"], rtol=1e-9, atol=0)
    host = coordinate_search(lambda tau, vary, cand: ensemble_nll_grid_numpy(raw, labels, tau, vary, cand), E, -1, r["tau_init"])
    print(f"host: tau {host['tau']}, sweeps {host['sweeps']}, after {host['nll_after']}")
    assert r["stopped_by_rule"] and host["stopped_by_rule"]
    sweep_rtol = 1e-7
    assert abs(r["nll_after"][-1] / host["nll_after"][-1] - 1) <= 10 * sweep_rtol
    # apply(): the model carries the vector, and the ensemble the engine forms under it is better calibrated
    assert ets.apply() == pytest.approx([float(t) for t in r["tau"]])
    assert m.exit_temperature == [float(t) for t in r["tau"]]
    after = last_row_nll()
    print(f"NLL of predict_ensemble's last row: {before:.3f} -> {after:.3f}")
    assert after < before
    monkeypatch.chdir(tmp_path)
    name = ets.save("t")
    assert name == "ensemble_temperature_t.npz"
    saved = np.load(name)
    for k, v in r.items():
        np.testing.assert_array_equal(saved[k], np.asarray(v))
    need = N * FIT_T * E * Cn * 4
    with pytest.raises(ValueError, match=str(need)):
        EnsembleTemperatureScaling(m, loader, gpu=0, mc_passes=FIT_T, seed=FIT_SEED, max_logit_bytes=need - 1).fit()
