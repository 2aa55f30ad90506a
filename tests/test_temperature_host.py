"""Per-exit temperature scaling, CPU side: the three C-ABI entry points are declared, the float64 restatements (nll_grid_numpy,
temper_logits) against direct torch float64 arithmetic, the deterministic search against scipy's bounded minimiser on inputs a dense scan
shows to be unimodal, and the host-side validation of temperatures (model, engine handle, C ABI)."""
import ctypes as C

import numpy as np
import pytest
import torch

from bayesnn_fpga_amd import _lib
from bayesnn_fpga_amd.engine import CompiledGraph, check_temperature
from bayesnn_fpga_amd.models.resnet18.resnet18 import ResNet18MC, ResNet18MCEarlyExit
from bayesnn_fpga_amd.train.calibration import TemperatureScaling, nll_grid_numpy, temper_logits, zoom_search
from tests.helpers import build_seeded

KW = dict(dropout_exit=True, dropout="block", dropout_p=0.25, out_dim=10)


def test_lib_declares_the_entry_points():
    for name in ("bmi_engine_set_temperature", "bmi_engine_get_temperature", "bmi_nll_temperature_grid", "bmi_nll_temperature_scratch_bytes"):
        assert name in _lib.EXPORTS
        assert hasattr(_lib.lib(), name)
    assert _lib.lib().bmi_nll_temperature_scratch_bytes(4, 250, 33) == 4 * 250 * 33 * 8
    assert _lib.ABI_VERSION == 600


def _torch_nll(logits, labels, tau_grid):
    """softmax -> mean over T -> -log -> sum, float64 torch."""
    l = torch.from_numpy(np.asarray(logits)).double()
    T, E, B, Cn = l.shape
    out = np.zeros(tau_grid.shape)
    y = torch.from_numpy(np.asarray(labels)).long()
    for e in range(E):
        for g in range(tau_grid.shape[1]):
            tau = float(np.float32(tau_grid[e, g]))
            p = torch.softmax(l[:, e] / tau, dim=-1).mean(0)
            out[e, g] = float(-torch.log(p[torch.arange(B), y]).sum())
    return out


@pytest.mark.parametrize("scale", [1.0, 30.0, 300.0])
def test_nll_grid_numpy_is_the_direct_computation(scale):
    """1e-12 relative against softmax / mean / -log in torch float64, logits up to +-300, tau from 0.05 to 20.  (Where the direct form's
    probability of the label underflows to 0 in EVERY sample it gives inf; the log-sum-exp form does not — those entries are only required
    to be finite and at least as large as the largest finite one.)"""
    rng = np.random.default_rng(int(scale))
    T, E, B, Cn = 7, 3, 40, 10
    logits = np.clip(rng.standard_normal((T, E, B, Cn)) * scale / 3, -scale, scale).astype(np.float32)
    labels = rng.integers(0, Cn, B)
    tau = np.exp(np.linspace(np.log(0.05), np.log(20.0), 9)).astype(np.float32)
    grid = np.stack([tau, tau[::-1], tau])
    got = nll_grid_numpy(logits, labels, grid)
    ref = _torch_nll(logits, labels, grid)
    assert np.isfinite(got).all()
    ok = np.isfinite(ref)
    assert ok.sum() >= ok.size // 2
    np.testing.assert_allclose(got[ok], ref[ok], rtol=1e-12, atol=0)
    if (~ok).any():
        assert got[~ok].min() >= 700.0          # -log of a double that underflowed: beyond 745 for at least one image


def test_nll_grid_numpy_rejects_bad_labels_and_shapes():
    logits = np.zeros((2, 2, 3, 5), np.float32)
    with pytest.raises(ValueError):
        nll_grid_numpy(logits, [0, 1, 5], np.ones((2, 1)))
    with pytest.raises(ValueError):
        nll_grid_numpy(logits, [0, 1, -1], np.ones((2, 1)))
    with pytest.raises(ValueError):
        nll_grid_numpy(logits, [0, 1, 2], np.ones((3, 1)))


def test_temper_logits_at_one_is_the_plain_softmax():
    rng = np.random.default_rng(3)
    logits = (rng.standard_normal((6, 4, 9, 10)) * 5).astype(np.float32)
    p = torch.softmax(torch.from_numpy(logits).double(), dim=-1).numpy()
    for tau in (1.0, [1.0] * 4, None):
        mean, var = temper_logits(logits, 1.0 if tau is None else tau)
        np.testing.assert_allclose(mean, p.mean(0), rtol=0, atol=1e-15)
        np.testing.assert_allclose(var, p.var(0), rtol=0, atol=1e-15)
    # per-exit temperatures act on their own exit, as the fp32 product the head forms
    mean, _ = temper_logits(logits, [0.5, 1.0, 2.5, 4.0])
    z = (logits[:, 2] * np.float32(1.0 / np.float64(np.float32(2.5)))).astype(np.float64)
    np.testing.assert_allclose(mean[2], torch.softmax(torch.from_numpy(z), dim=-1).mean(0).numpy(), rtol=0, atol=1e-15)
    np.testing.assert_allclose(mean[1], p.mean(0)[1], rtol=0, atol=1e-15)


def _synthetic_problem(n=1000, T=10, Cn=10, tau_star=3.0, seed=0):
    """Peaky synthetic logits [T, 1, N, C] with teacher labels drawn from the model's own predictive tempered at tau_star."""
    rng = np.random.default_rng(seed)
    base = rng.standard_normal((n, 1, Cn)) * 6
    logits = np.transpose(base + rng.standard_normal((n, T, Cn)), (1, 0, 2))[:, None].astype(np.float32)
    mean, _ = temper_logits(logits, tau_star)
    teacher = np.array([rng.choice(Cn, p=p / p.sum()) for p in mean[0]])
    uniform = rng.integers(0, Cn, n)
    return logits, teacher, uniform


def test_zoom_search_against_scipy_on_a_unimodal_objective():
    from scipy.optimize import minimize_scalar
    logits, teacher, uniform = _synthetic_problem()
    f = lambda tau: nll_grid_numpy(logits, teacher, tau)
    # a dense scan shows ONE local minimum inside the bracket: a multimodal input cannot hide a failure of the search
    scan = np.exp(np.linspace(np.log(0.05), np.log(20.0), 2000))
    v = f(scan[None].astype(np.float32))[0]
    interior_minima = int(np.sum((v[1:-1] < v[:-2]) & (v[1:-1] <= v[2:])))
    assert interior_minima == 1 and v.argmin() not in (0, len(v) - 1)
    calls = []
    r = zoom_search(lambda tau: (calls.append(tau.shape), f(tau))[1], 1, rtol=1e-4)
    opt = minimize_scalar(lambda t: float(f(np.array([[t]]))[0, 0]), bounds=(0.05, 20.0), method="bounded", options={"xatol": 1e-6})
    assert abs(r["tau"][0] - opt.x) <= 2e-4 * opt.x, (r["tau"][0], opt.x)
    assert abs(r["tau"][0] - 3.0) < 0.3                       # the teacher's temperature, to sampling noise at n = 1000
    assert not r["at_bound"][0] and r["rounds"] <= 8
    assert r["nll_after"][0] <= r["nll_before"][0]
    assert abs(r["nll_before"][0] - f(np.ones((1, 1)))[0, 0]) <= 1e-9 * r["nll_before"][0]
    assert calls[0] == (1, 34) and all(c == (1, 33) for c in calls[1:])       # the grid plus tau = 1 exactly in round one
    # uniform random labels on peaky logits: the optimum runs to the upper end of the bracket, and at_bound says so
    r2 = zoom_search(lambda tau: nll_grid_numpy(logits, uniform, tau), 1)
    assert r2["at_bound"][0] and r2["tau"][0] == 20.0
    assert r2["nll_after"][0] <= r2["nll_before"][0]


def test_zoom_search_runs_exits_independently_and_hits_exact_bracket_ends():
    """Two analytic objectives in one call: (log tau - log 2)^2 and a monotone one; the first grid's ends are the bracket's ends themselves."""
    seen = []

    def f(tau):
        seen.append(tau.copy())
        return np.stack([(np.log(tau[0]) - np.log(2.0)) ** 2, -np.log(tau[1])])
    r = zoom_search(f, 2, bracket=(0.05, 20.0), grid=33, rtol=1e-4)
    lo32, hi32 = float(np.float32(0.05)), 20.0
    assert seen[0][0, 0] == lo32 and seen[0][0, 32] == hi32 and seen[0][0, 33] == 1.0
    assert abs(r["tau"][0] - 2.0) <= 2e-4 * 2.0 and not r["at_bound"][0]
    assert r["tau"][1] == hi32 and r["at_bound"][1]
    assert all(np.all(s.astype(np.float32).astype(np.float64) == s) for s in seen)      # float32-representable candidates


@pytest.mark.parametrize("bad", [0.0, -1.0, float("nan"), float("inf"), [1.0, 2.0], [1.0, 1.0, 0.0, 1.0], [1.0, float("nan"), 1.0, 1.0], 1e-46])
def test_validation_errors_on_the_host(bad):
    m = build_seeded(ResNet18MCEarlyExit, KW)
    with pytest.raises(ValueError):
        m.set_exit_temperature(bad)
    assert m.exit_temperature is None
    with pytest.raises(ValueError):
        check_temperature(bad, 4)


def test_model_attribute_is_a_plain_list_and_engines_inherit_it():
    m = build_seeded(ResNet18MCEarlyExit, KW)
    assert m.exit_temperature is None
    m.set_exit_temperature(2.0)
    assert m.exit_temperature == [2.0] * 4 and all(type(v) is float for v in m.exit_temperature)
    m.set_exit_temperature(torch.tensor([0.5, 1.0, 2.5, 4.0]))
    assert m.exit_temperature == [0.5, 1.0, 2.5, 4.0]
    g = CompiledGraph(m, "cpu", 4)                         # host half of the engine: no GPU call
    assert g.temperature == [0.5, 1.0, 2.5, 4.0]
    g.set_temperature(None)
    assert g.temperature == [1.0] * 4
    with pytest.raises(ValueError):
        g.set_temperature([1.0, 2.0])
    g.set_temperature([1.0] * 4)
    assert g.temperature == [1.0] * 4
    m.set_exit_temperature(None)
    assert m.exit_temperature is None
    single = build_seeded(ResNet18MC, KW)
    single.set_exit_temperature([1.5])
    assert CompiledGraph(single, "cpu", 2).temperature == [1.5]


def test_c_abi_validation():
    m = build_seeded(ResNet18MCEarlyExit, KW)
    g = CompiledGraph(m, "cpu", 4)
    lib = g.lib
    arr = lambda *v: (C.c_float * len(v))(*v)
    assert lib.bmi_engine_set_temperature(g.handle, arr(1, 2, 3, 4), 4) == _lib.BMI_OK
    for bad, n in ((arr(1, 2, 3), 3), (arr(1, 2, 3, 4, 5), 5), (arr(1, 0, 1, 1), 4), (arr(1, -2, 1, 1), 4), (arr(1, float("nan"), 1, 1), 4),
                   (arr(1, float("inf"), 1, 1), 4)):
        assert lib.bmi_engine_set_temperature(g.handle, bad, n) == -22
    out = arr(0, 0, 0, 0)
    assert lib.bmi_engine_get_temperature(g.handle, out, 4) == _lib.BMI_OK and list(out) == [1.0, 2.0, 3.0, 4.0]      # a refused call changes nothing
    assert lib.bmi_engine_get_temperature(g.handle, out, 3) == -22
    assert lib.bmi_engine_set_temperature(g.handle, None, 0) == _lib.BMI_OK
    assert lib.bmi_engine_get_temperature(g.handle, out, 4) == _lib.BMI_OK and list(out) == [1.0] * 4
    assert lib.bmi_engine_set_temperature(None, arr(1, 1, 1, 1), 4) == -22
    # the fit entry point validates on the host before any launch
    assert lib.bmi_nll_temperature_grid(None, 1, 1, 1, 1, None, None, 1, None, None, 0, None) == -22
    assert lib.bmi_nll_temperature_scratch_bytes(0, 1, 1) == 0


def test_temperature_scaling_budget_and_label_checks_need_no_gpu():
    """Both checks run before anything touches the device: the logit budget (named in the message) and the label range."""
    m = build_seeded(ResNet18MCEarlyExit, KW)
    x, y = torch.zeros(8, 3, 32, 32), torch.zeros(8, dtype=torch.int64)
    ts = TemperatureScaling(m, [(x, y)], gpu=-1, mc_passes=10, max_logit_bytes=8 * 10 * 4 * 10 * 4 - 1)
    with pytest.raises(ValueError, match=str(8 * 10 * 4 * 10 * 4)):
        ts.fit()
    y_bad = y.clone()
    y_bad[3] = 10
    with pytest.raises(ValueError, match="labels"):
        TemperatureScaling(m, [(x, y_bad)], gpu=-1, mc_passes=10).fit()
    with pytest.raises(RuntimeError):
        ts.apply()
