"""Joint temperature fit of the exit ensembles, CPU side: the two C-ABI entry points are declared and validate on the host, the float64
restatement (ensemble_nll_grid_numpy) against direct torch float64 arithmetic, against the reference's ensemble softmax on the goldens and
against the per-exit objective where the two coincide, and coordinate_search over that restatement."""
import os
import re

import numpy as np
import pytest
import torch

from bayesnn_fpga_amd import _lib
from bayesnn_fpga_amd.engine import vary_mask
from bayesnn_fpga_amd.train import EnsembleTemperatureScaling, TemperatureScaling
from bayesnn_fpga_amd.train.calibration import coordinate_search, ensemble_nll_grid_numpy, nll_grid_numpy, temper_logits, zoom_search

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
NAMES = ("bmi_nll_ensemble_temperature_grid", "bmi_nll_ensemble_temperature_scratch_bytes")


# ---- 1. entry points --------------------------------------------------------------------------------------------------------------
def test_lib_declares_the_entry_points_and_validates_on_the_host():
    lib = _lib.lib()
    for name in NAMES:
        assert name in _lib.EXPORTS
        assert hasattr(lib, name)
    assert lib.bmi_nll_ensemble_temperature_scratch_bytes(4, 250, 33) == 4 * 250 * 33 * 8
    assert lib.bmi_nll_ensemble_temperature_scratch_bytes(0, 1, 1) == 0
    assert _lib.ABI_VERSION == 600 and lib.bmi_version() == 600
    assert lib.bmi_nll_ensemble_temperature_grid(None, 1, 1, 1, 1, None, None, 0, None, 1, None, None, 0, None) == -22
    # a mask bit at or above E, every pointer non-null (never dereferenced: the call is refused before any HIP call)
    buf = (np.zeros(64, np.float64)).ctypes.data
    E = 4
    for mask in (1 << E, 1 << 31, (1 << E) | 1):
        assert lib.bmi_nll_ensemble_temperature_grid(buf, 1, E, 1, 2, buf, buf, mask, buf, 1, buf, buf, 1 << 20, None) == -22
    for bad in (dict(T=0), dict(E=0), dict(B=0), dict(C=0), dict(G=0)):
        a = dict(T=1, E=E, B=1, C=2, G=1)
        a.update(bad)
        assert lib.bmi_nll_ensemble_temperature_grid(buf, a["T"], a["E"], a["B"], a["C"], buf, buf, 0, buf, a["G"], buf, buf, 1 << 20, None) == -22


def test_binding_mirrors_the_header_limits_and_vary_mask():
    hdr = open(os.path.join(os.path.dirname(GOLDEN), "..", "include", "bayesnn_fpga_amd.h")).read()
    assert int(re.search(r"#define BMI_NLL_ENS_SLAB (\d+)", hdr).group(1)) == _lib.NLL_ENS_SLAB
    assert int(re.search(r"#define BMI_NLL_ENS_ROWS (\d+)", hdr).group(1)) == _lib.NLL_ENS_ROWS
    assert vary_mask(None, 4) == 0 and vary_mask(2, 4) == 4 and vary_mask([0, 3], 4) == 9 and vary_mask(range(4), 4) == 15
    for bad in (4, -1, [0, 4]):
        with pytest.raises(ValueError):
            vary_mask(bad, 4)
    assert issubclass(EnsembleTemperatureScaling, TemperatureScaling)


# ---- 2. the restatement against direct arithmetic -----------------------------------------------------------------------------------
def _torch_ensemble_nll(logits, labels, tau, vary, cand):
    """softmax(l / tau) -> mean over exits 0..e and T -> -log -> sum, float64 torch."""
    l = torch.from_numpy(np.asarray(logits)).double()
    T, E, B, Cn = l.shape
    y = torch.from_numpy(np.asarray(labels)).long()
    out = np.zeros((E, len(cand)))
    for g in range(len(cand)):
        t = [float(np.float32(cand[g])) if i in vary else float(np.float32(tau[i])) for i in range(E)]
        p = torch.stack([torch.softmax(l[:, i] / t[i], dim=-1) for i in range(E)], dim=1)       # [T, E, B, C]
        for e in range(E):
            q = p[:, :e + 1].mean(dim=(0, 1))
            out[e, g] = float(-torch.log(q[torch.arange(B), y]).sum())
    return out


@pytest.mark.parametrize("vary", [(), (0,), (1,), (2,), (0, 1, 2)], ids=["none", "0", "1", "2", "all"])
@pytest.mark.parametrize("scale", [1.0, 30.0, 300.0])
def test_ensemble_nll_grid_numpy_is_the_direct_computation(scale, vary):
    """1e-12 relative against softmax / mean / -log in torch float64, logits up to +-300, tau and candidates from 0.05 to 20, where the
    direct form is finite — at least half of the entries; where the label's probability underflows to 0 in every member the direct form
    gives inf and the log-sum-exp form a finite value of at least 700 (-log of a double that underflowed is beyond 745)."""
    rng = np.random.default_rng(int(scale))
    T, E, B, Cn = 7, 3, 40, 10
    logits = np.clip(rng.standard_normal((T, E, B, Cn)) * scale / 3, -scale, scale).astype(np.float32)
    labels = rng.integers(0, Cn, B)
    cand = np.exp(np.linspace(np.log(0.05), np.log(20.0), 9)).astype(np.float32)
    tau = np.array([0.05, 1.3, 20.0], np.float32)
    got = ensemble_nll_grid_numpy(logits, labels, tau, list(vary) or None, cand)
    ref = _torch_ensemble_nll(logits, labels, tau, vary, cand)
    assert got.shape == (E, 9) and np.isfinite(got).all()
    ok = np.isfinite(ref)
    print(f"scale {scale} vary {vary}: {int(ok.sum())} of {ok.size} entries finite in the direct form")
    assert ok.sum() >= ok.size // 2 + ok.size % 2
    np.testing.assert_allclose(got[ok], ref[ok], rtol=1e-12, atol=0)
    if (~ok).any():
        assert got[~ok].min() >= 700.0


def test_ensemble_nll_grid_numpy_rejects_bad_input():
    logits = np.zeros((2, 2, 3, 5), np.float32)
    with pytest.raises(ValueError):
        ensemble_nll_grid_numpy(logits, [0, 1, 5], [1, 1], None, [1.0])
    with pytest.raises(ValueError):
        ensemble_nll_grid_numpy(logits, [0, 1, 2], [1, 1, 1], None, [1.0])
    with pytest.raises(ValueError):
        ensemble_nll_grid_numpy(logits, [0, 1, 2], [1, 1], 2, [1.0])


# ---- 3. pinned to the reference -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["resnet18_block_exit", "resnet18_exit_only", "resnet18_mask4_block_exit"])
def test_rows_at_one_are_the_reference_ensemble_likelihood(name):
    """At tau = 1, labels arange(B) % C: row e = -sum_b log go_ensemble_output_sm[e][b, y_b] within 1e-6 relative (the reference's softmax
    is fp32, eps 6e-8; an order of margin over it)."""
    g = np.load(os.path.join(GOLDEN, name + ".npz"))
    logits, sm = g["logits"], g["go_ensemble_output_sm"]
    T, E, B, Cn = logits.shape
    y = np.arange(B) % Cn
    ref = np.array([-np.log(sm[e][np.arange(B), y]).sum() for e in range(E)])
    worst = 0.0
    for vary, tau in ((None, 1.0), (range(E), [0.3, 2.0, 5.0, 0.7]), (1, np.ones(E))):
        got = ensemble_nll_grid_numpy(logits, y, tau, vary, [1.0])[:, 0]
        worst = max(worst, float(np.abs(got / ref - 1).max()))
        np.testing.assert_allclose(got, ref, rtol=1e-6, atol=0)
    print(f"{name}: worst relative difference to the reference {worst:.2e}")


# ---- 4. consistent with the per-exit objective --------------------------------------------------------------------------------------
def test_row_zero_and_one_exit_are_the_per_exit_objective():
    rng = np.random.default_rng(11)
    logits = (rng.standard_normal((5, 3, 30, 10)) * 8).astype(np.float32)
    labels = rng.integers(0, 10, 30)
    cand = np.exp(np.linspace(np.log(0.05), np.log(20.0), 9)).astype(np.float32)
    row0 = ensemble_nll_grid_numpy(logits, labels, [0.7, 1.1, 2.0], 0, cand)[0]
    per_exit = nll_grid_numpy(logits, labels, np.stack([cand] * 3))
    np.testing.assert_allclose(row0, per_exit[0], rtol=1e-12, atol=0)
    for e in range(3):
        one = ensemble_nll_grid_numpy(logits[:, e:e + 1], labels, 1.0, 0, cand)
        assert one.shape == (1, 9)
        np.testing.assert_allclose(one[0], per_exit[e], rtol=1e-12, atol=0)


# ---- 5. coordinate_search -----------------------------------------------------------------------------------------------------------
def _small_set(T=6, E=3, B=300, Cn=10, seed=2):
    """Seeded logits whose last exit is over-confident, teacher labels drawn from the full ensemble's predictive at tau = 2."""
    rng = np.random.default_rng(seed)
    base = rng.standard_normal((B, Cn)) * 3
    logits = np.stack([np.stack([(base + rng.standard_normal((B, Cn))) * (1.0 + 1.5 * i) for i in range(E)]) for _ in range(T)]).astype(np.float32)
    mean, _ = temper_logits(logits, 2.0)
    q = mean.mean(0)
    labels = np.array([rng.choice(Cn, p=p / p.sum()) for p in q])
    return logits, labels


def test_coordinate_search_on_the_host():
    logits, labels = _small_set()
    E = 3
    calls = []

    def f(tau, vary, cand):
        calls.append((np.array(tau), vary, np.array(cand)))
        return ensemble_nll_grid_numpy(logits, labels, tau, vary, cand)
    r = coordinate_search(f, E, -1, [1.0, 0.5, 4.0])
    print(f"vector: tau {r['tau']}, nll {r['nll_init']} -> {r['nll_after']}, sweeps {r['sweeps']}, trace {r['trace']}")
    assert r["stopped_by_rule"] and 1 <= r["sweeps"] <= 50 and len(r["trace"]) == r["sweeps"]
    assert np.all(np.diff(np.concatenate([[r["nll_init"][-1]], r["trace"]])) <= 0)
    assert r["nll_after"][-1] <= r["nll_init"][-1]
    np.testing.assert_allclose(r["nll_after"][-1], r["trace"][-1], rtol=1e-12)
    np.testing.assert_allclose(r["nll_after"], ensemble_nll_grid_numpy(logits, labels, r["tau"], None, [1.0])[:, 0], rtol=1e-12)
    np.testing.assert_allclose(r["nll_init"], ensemble_nll_grid_numpy(logits, labels, [1.0, 0.5, 4.0], None, [1.0])[:, 0], rtol=1e-12)
    assert r["nll_after"][-1] < ensemble_nll_grid_numpy(logits, labels, 1.0, None, [1.0])[-1, 0]
    assert np.all(r["tau"].astype(np.float32).astype(np.float64) == r["tau"])
    # every coordinate step had the coordinate's current value among its candidates, in every round
    steps = [(t, v, c) for t, v, c in calls if v is not None]
    assert steps and all(t[v] in c for t, v, c in steps)
    # a lower target: the exits above it keep their init value, and are not members of the row that is searched
    r1 = coordinate_search(f, E, 1, [1.0, 0.5, 4.0])
    assert r1["tau"][2] == 4.0 and not r1["at_bound"][2]
    assert r1["nll_after"][1] <= r1["nll_init"][1] and np.all(np.diff(r1["trace"]) <= 0)
    r0 = coordinate_search(f, E, 0, 1.0)
    assert r0["tau"][1] == 1.0 and r0["tau"][2] == 1.0
    z = zoom_search(lambda tau: nll_grid_numpy(logits[:, :1], labels, tau), 1)
    assert abs(r0["tau"][0] / z["tau"][0] - 1) <= 2e-4          # one member: the per-exit fit
    # shared: one temperature for exits 0..target
    rs = coordinate_search(f, E, -1, 1.0, mode="shared")
    assert rs["tau"][0] == rs["tau"][1] == rs["tau"][2] and rs["sweeps"] == 1 and rs["stopped_by_rule"]
    assert rs["nll_after"][-1] <= rs["nll_init"][-1]
    rs1 = coordinate_search(f, E, 1, [1.0, 1.0, 4.0], mode="shared")
    assert rs1["tau"][0] == rs1["tau"][1] and rs1["tau"][2] == 4.0
    assert rs1["nll_after"][1] <= rs1["nll_init"][1]
    assert r["nll_after"][-1] <= rs["nll_after"][-1] * (1 + 1e-4)      # the vector has the shared temperature's freedom and more (to the searches' rtol)
    with pytest.raises(ValueError):
        coordinate_search(f, E, 3, 1.0)
    with pytest.raises(ValueError):
        coordinate_search(f, E, -1, 1.0, mode="matrix")
    with pytest.raises(ValueError):
        coordinate_search(f, E, -1, [1.0, 0.0, 1.0])


def test_zoom_search_default_is_unchanged_and_include_is_a_candidate():
    """The default zoom_search (no include) on the existing scipy case: the same calls and the same answer as scipy's bounded minimiser, as
    tests/test_temperature_host.py holds it to; with include the value is among the candidates of every round and bounds the result."""
    from scipy.optimize import minimize_scalar
    from tests.test_temperature_host import _synthetic_problem
    logits, teacher, _ = _synthetic_problem()
    f = lambda tau: nll_grid_numpy(logits, teacher, tau)        # noqa: E731
    calls = []
    r = zoom_search(lambda tau: (calls.append(tau.copy()), f(tau))[1], 1, rtol=1e-4)
    opt = minimize_scalar(lambda t: float(f(np.array([[t]]))[0, 0]), bounds=(0.05, 20.0), method="bounded", options={"xatol": 1e-6})
    assert abs(r["tau"][0] - opt.x) <= 2e-4 * opt.x
    assert calls[0].shape == (1, 34) and all(c.shape == (1, 33) for c in calls[1:]) and calls[0][0, -1] == 1.0
    inc = []
    ri = zoom_search(lambda tau: (inc.append(tau.copy()), f(tau))[1], 1, rtol=1e-4, include=2.875)
    assert inc[0].shape == (1, 35) and all(c.shape == (1, 34) for c in inc[1:]) and all(2.875 in c[0] for c in inc)
    assert inc[0][0, -1] == 1.0 and ri["nll_before"][0] == r["nll_before"][0]
    assert ri["nll_after"][0] <= f(np.array([[2.875]]))[0, 0]
    assert abs(ri["tau"][0] - opt.x) <= 2e-4 * opt.x
    # a point far better than anything on the grid, outside the bracket: the argmin keeps it
    g = lambda tau: np.where(tau == 25.0, -1.0, (np.log(tau) - np.log(2.0)) ** 2)      # noqa: E731
    assert zoom_search(g, 1, include=25.0)["tau"][0] == 25.0


def test_ensemble_fit_budget_check_needs_no_gpu():
    from bayesnn_fpga_amd.models.resnet18.resnet18 import ResNet18MCEarlyExit
    from tests.helpers import build_seeded
    m = build_seeded(ResNet18MCEarlyExit, dict(dropout_exit=True, dropout="block", dropout_p=0.25, out_dim=10))
    x, y = torch.zeros(8, 3, 32, 32), torch.zeros(8, dtype=torch.int64)
    ets = EnsembleTemperatureScaling(m, [(x, y)], gpu=-1, mc_passes=10, max_logit_bytes=8 * 10 * 4 * 10 * 4 - 1)
    with pytest.raises(ValueError, match=str(8 * 10 * 4 * 10 * 4)):
        ets.fit()
    with pytest.raises(RuntimeError):
        ets.save("x")
