"""Vector scaling without a GPU: the float64 restatement of the fit objective (value against nll_grid_numpy, gradient against central
differences), the L-BFGS, check_vector_scaling and the model setters (shapes, broadcasting, mutual exclusion with the temperature, pickling),
the ctypes bindings and the C ABI's host-side validation (no call reaches a kernel)."""
import copy
import ctypes as C
import pickle

import numpy as np
import pytest
import torch

from bayesnn_fpga_amd import _lib
from bayesnn_fpga_amd.engine import CompiledGraph, check_vector_scaling
from bayesnn_fpga_amd.models.resnet18.resnet18 import ResNet18MCEarlyExit
from bayesnn_fpga_amd.train.calibration import lbfgs_minimize, nll_grid_numpy, nll_vector_numpy, scale_logits, temper_logits
from bayesnn_fpga_amd.train.uncertainty import decompose_ensemble_logits
from tests.helpers import build_seeded

KW = dict(dropout_exit=True, dropout="block", dropout_p=0.25, out_dim=10)
NEW = ("bmi_engine_set_vector_scaling", "bmi_ensemble_moments_vector", "bmi_nll_vector_scratch_bytes", "bmi_nll_vector_scaling_grad")


def _problem(C_, T=10, E=2, B=50, seed=0):
    rng = np.random.default_rng(seed + C_)
    logits = (rng.standard_normal((T, E, B, C_)) * 3.0).astype(np.float32)
    labels = rng.integers(0, C_, B)
    return logits, labels, rng.uniform(0.4, 2.2, (E, C_)), rng.uniform(-1.0, 1.0, (E, C_))


@pytest.mark.parametrize("C_", [10, 37])
def test_gradient_against_central_differences(C_):
    """Every entry of both gradients against central differences of nll_vector_numpy's own value (float64, h = 1e-5): within 1e-6 of the
    largest gradient entry (the truncation error h^2 f''' / 6 and the rounding error eps f / h are both orders below); sum_c g_bias = 0."""
    logits, labels, a, b = _problem(C_)
    E = a.shape[0]
    f, ga, gb = nll_vector_numpy(logits, labels, a, b)
    assert f.shape == (E,) and ga.shape == gb.shape == (E, C_)
    h, fd = 1e-5, [np.zeros((E, C_)), np.zeros((E, C_))]
    for which in (0, 1):
        for c in range(C_):
            p, m = [a.copy(), b.copy()], [a.copy(), b.copy()]
            p[which][:, c] += h                  # (the exits are independent problems: one perturbation serves all of them)
            m[which][:, c] -= h
            fd[which][:, c] = (nll_vector_numpy(logits, labels, *p)[0] - nll_vector_numpy(logits, labels, *m)[0]) / (2 * h)
    big = max(float(np.abs(ga).max()), float(np.abs(gb).max()))
    err = max(float(np.abs(fd[0] - ga).max()), float(np.abs(fd[1] - gb).max())) / big
    print(f"C {C_}: relative error against central differences {err:.2e}, |sum g_bias| {np.abs(gb.sum(1)).max():.2e}")
    assert err <= 1e-6
    assert np.abs(gb.sum(1)).max() <= 1e-10


@pytest.mark.parametrize("C_", [10, 37])
def test_value_equals_the_temperature_objective_on_a_uniform_scale(C_):
    logits, labels, _, _ = _problem(C_)
    tau = np.array([[0.7], [1.9]], dtype=np.float32)
    inv = 1.0 / tau.astype(np.float64)
    f = nll_vector_numpy(logits, labels, np.repeat(inv, C_, axis=1), np.zeros((2, C_)))[0]
    np.testing.assert_allclose(f, nll_grid_numpy(logits, labels, tau)[:, 0], rtol=1e-12, atol=0)


def test_scale_logits_is_temper_logits_on_a_uniform_scale_and_feeds_the_ensemble_restatement():
    logits = _problem(10, T=7, E=4, B=3)[0]
    tau = [0.5, 1.0, 1.9, 3.1]
    inv = (1.0 / np.asarray(tau, np.float32).astype(np.float64)).astype(np.float32)
    a = np.repeat(inv[:, None], 10, axis=1)
    for got, want in zip(scale_logits(logits, a), temper_logits(logits, tau)):
        assert np.array_equal(got, want)
    r, w = decompose_ensemble_logits(logits, scale=a), decompose_ensemble_logits(logits, tau)
    assert all(np.array_equal(r[k], w[k]) for k in w)
    with pytest.raises(ValueError):
        decompose_ensemble_logits(logits, tau, scale=a)
    rng = np.random.default_rng(1)
    a, b = rng.uniform(0.4, 2.2, (4, 10)), rng.uniform(-1, 1, (4, 10))
    mean, _ = scale_logits(logits, a, b)
    np.testing.assert_allclose(decompose_ensemble_logits(logits, scale=a, bias=b)["mean"][0], mean[0], rtol=0, atol=1e-15)


def test_lbfgs_reaches_the_minimiser_of_convex_quadratics_monotonically():
    rng = np.random.default_rng(3)
    P, D = 3, 8
    A = []
    for _ in range(P):
        q = np.linalg.qr(rng.standard_normal((D, D)))[0]
        A.append(q @ np.diag(rng.uniform(0.5, 30.0, D)) @ q.T)
    b = rng.standard_normal((P, D))
    calls = []

    def fun(x):
        calls.append(x.copy())
        return (np.array([0.5 * x[p] @ A[p] @ x[p] - b[p] @ x[p] for p in range(P)]), np.stack([A[p] @ x[p] - b[p] for p in range(P)]))
    r = lbfgs_minimize(fun, np.zeros((P, D)), max_iter=200, gtol=1e-8)
    want = np.stack([np.linalg.solve(A[p], b[p]) for p in range(P)])
    assert r["converged"].all() and r["n_eval"] == len(calls)
    np.testing.assert_allclose(r["x"], want, rtol=0, atol=1e-7)
    tr = np.stack(r["trace"])
    assert (tr[1:] <= tr[:-1]).all() and (tr[-1] < tr[0]).all()
    np.testing.assert_array_equal(r["f"], tr[-1])
    again = lbfgs_minimize(fun, np.zeros((P, D)), max_iter=200, gtol=1e-8)
    assert np.array_equal(again["x"], r["x"])                                   # deterministic


def test_check_vector_scaling():
    a, b = check_vector_scaling(np.arange(1, 11), None, 4, 10)
    assert a.shape == b.shape == (4, 10) and a.dtype == b.dtype == np.float32 and a.flags.c_contiguous
    assert np.array_equal(a, np.broadcast_to(np.arange(1, 11, dtype=np.float32), (4, 10))) and not b.any()
    a, b = check_vector_scaling(torch.full((4, 10), -2.0), np.ones(10), 4, 10)       # no sign constraint
    assert (a == -2).all() and (b == 1).all()
    assert check_vector_scaling(None, None, 4, 10) == (None, None)
    for bad in (np.ones(9), np.ones((3, 10)), np.ones((4, 10, 1)), 1.0, np.ones((10, 4))):
        with pytest.raises(ValueError):
            check_vector_scaling(bad, None, 4, 10)
        with pytest.raises(ValueError):
            check_vector_scaling(np.ones(10), bad, 4, 10)
    for v in (np.nan, np.inf, -np.inf, 1e39):
        bad = np.ones((4, 10))
        bad[2, 3] = v
        with pytest.raises(ValueError):
            check_vector_scaling(bad, None, 4, 10)
        with pytest.raises(ValueError):
            check_vector_scaling(np.ones(10), bad, 4, 10)
    with pytest.raises(ValueError):
        check_vector_scaling(None, np.ones(10), 4, 10)


def test_model_setters_exclude_each_other_survive_pickling_and_drop_engines():
    m = build_seeded(ResNet18MCEarlyExit, KW)
    assert m.exit_vector_scaling is None
    m._engines["stale"] = object()
    m.set_exit_vector_scaling(np.linspace(0.5, 2.0, 10), np.linspace(-1, 1, 40).reshape(4, 10))
    a, b = m.exit_vector_scaling
    assert m._engines == {} and type(a) is np.ndarray and a.dtype == b.dtype == np.float32 and a.shape == b.shape == (4, 10)
    with pytest.raises(ValueError):
        m.set_exit_temperature([0.5, 1.0, 2.0, 4.0])
    with pytest.raises(ValueError):
        m.set_exit_temperature(2.0)
    assert m.exit_temperature is None
    m.set_exit_temperature(None)                                                # clearing is always allowed
    for m2 in (pickle.loads(pickle.dumps(m)), copy.deepcopy(m)):
        a2, b2 = m2.exit_vector_scaling
        assert type(a2) is np.ndarray and np.array_equal(a2, a) and np.array_equal(b2, b)
    m.set_exit_vector_scaling(None)
    assert m.exit_vector_scaling is None
    m.set_exit_temperature([0.5, 1.0, 2.0, 4.0])
    with pytest.raises(ValueError):
        m.set_exit_vector_scaling(np.ones(10))
    assert m.exit_vector_scaling is None and m.exit_temperature == [0.5, 1.0, 2.0, 4.0]
    m.set_exit_temperature(None)
    m.set_exit_vector_scaling(np.ones(10))
    assert m.exit_vector_scaling is not None


def test_lib_declares_the_entry_points_and_the_abi_version_stays():
    for name in NEW:
        assert name in _lib.EXPORTS
        assert hasattr(_lib.lib(), name)
    assert _lib.ABI_VERSION == 600 and _lib.lib().bmi_version() == 600


def test_c_abi_validation():
    """Null handles, wrong counts, the mutual exclusion with the temperature in both directions, null pointers and unsupported shapes:
    decided on the host, before any launch (the pointers are never dereferenced)."""
    g = CompiledGraph(build_seeded(ResNet18MCEarlyExit, KW), "cpu", 4)
    lib, fake = g.lib, C.c_void_p(4096)
    INVALID, UNSUPPORTED, NOMEM = -22, -95, -12
    assert (_lib.BMI_OK, INVALID) == (0, -22)
    assert lib.bmi_engine_set_vector_scaling(None, fake, fake, 4, 10) == INVALID
    assert lib.bmi_engine_set_vector_scaling(g.handle, fake, None, 4, 10) == INVALID
    for E, Cd in ((3, 10), (5, 10), (4, 9), (4, 100), (0, 0)):
        assert lib.bmi_engine_set_vector_scaling(g.handle, fake, fake, E, Cd) == INVALID
    assert lib.bmi_engine_set_vector_scaling(g.handle, fake, fake, 4, 10) == _lib.BMI_OK
    tau = (C.c_float * 4)(0.5, 1.0, 2.0, 4.0)
    ones = (C.c_float * 4)(1.0, 1.0, 1.0, 1.0)
    assert lib.bmi_engine_set_temperature(g.handle, tau, 4) == INVALID           # a scaling is set
    assert lib.bmi_engine_set_temperature(g.handle, ones, 4) == _lib.BMI_OK      # all ones is off
    assert lib.bmi_engine_set_temperature(g.handle, None, 0) == _lib.BMI_OK
    assert lib.bmi_engine_set_vector_scaling(g.handle, None, None, 0, 0) == _lib.BMI_OK
    assert lib.bmi_engine_set_temperature(g.handle, tau, 4) == _lib.BMI_OK
    assert lib.bmi_engine_set_vector_scaling(g.handle, fake, fake, 4, 10) == INVALID       # a temperature is in force
    assert lib.bmi_engine_set_vector_scaling(g.handle, None, None, 0, 0) == _lib.BMI_OK    # clearing is always allowed
    assert lib.bmi_engine_set_temperature(g.handle, None, 0) == _lib.BMI_OK
    # the stand-alone ensemble entry
    assert lib.bmi_ensemble_moments_vector(None, 1, 1, 1, 1, fake, fake, None, fake, fake, fake, None) == INVALID
    assert lib.bmi_ensemble_moments_vector(fake, 1, 1, 1, 1, None, fake, None, fake, fake, fake, None) == INVALID
    assert lib.bmi_ensemble_moments_vector(fake, 1, 1, 1, 1, fake, None, None, fake, fake, fake, None) == INVALID
    assert lib.bmi_ensemble_moments_vector(fake, 0, 1, 1, 1, fake, fake, None, fake, fake, fake, None) == INVALID
    assert lib.bmi_ensemble_moments_vector(fake, 2, 33, 2, 10, fake, fake, None, fake, fake, fake, None) == UNSUPPORTED
    assert lib.bmi_ensemble_moments_vector(fake, 2, 2, 2, 129, fake, fake, fake, fake, fake, fake, None) == UNSUPPORTED
    # the fit entry
    assert lib.bmi_nll_vector_scratch_bytes(4, 250, 100) == 4 * 250 * 201 * 8
    assert lib.bmi_nll_vector_scratch_bytes(0, 250, 100) == 0 and lib.bmi_nll_vector_scratch_bytes(4, 250, 0) == 0
    ok = [fake, 10, 4, 7, 10, fake, fake, fake, fake, fake, fake, fake, 4 * 7 * 21 * 8, None]
    for i in (0, 5, 6, 7, 8, 9, 10, 11):
        args = list(ok)
        args[i] = None
        assert lib.bmi_nll_vector_scaling_grad(*args) == INVALID, i
    for i in (1, 2, 3, 4):
        args = list(ok)
        args[i] = 0
        assert lib.bmi_nll_vector_scaling_grad(*args) == INVALID, i
    args = list(ok)
    args[12] -= 1
    assert lib.bmi_nll_vector_scaling_grad(*args) == NOMEM
    args = list(ok)
    args[4], args[12] = 257, 4 * 7 * 515 * 8
    assert lib.bmi_nll_vector_scaling_grad(*args) == UNSUPPORTED
