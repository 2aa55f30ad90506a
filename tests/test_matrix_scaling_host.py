"""Matrix scaling without a GPU: check_matrix_scaling and the model setters (shapes, broadcasting, the three-way exclusion of the
calibration maps, pickling), the ctypes bindings and the C ABI's host-side validation (no call reaches a kernel), the fp32 restatement of
the head's arithmetic (a diagonal matrix is vector scaling bit for bit, a permutation matrix permutes the classes), the float64 restatement
of the fit objective (central differences, the diagonal anchor, the softmax gauge), the ODIR penalty, a numpy-only fit on a banded-teacher
problem, and VectorScaling's bias_l2 = 0 path."""
import copy
import ctypes as C
import pickle

import numpy as np
import pytest
import torch

from bayesnn_fpga_amd import _lib
from bayesnn_fpga_amd.engine import CompiledGraph, check_matrix_scaling
from bayesnn_fpga_amd.models.resnet18.resnet18 import ResNet18MCEarlyExit
from bayesnn_fpga_amd.train import calibration
from bayesnn_fpga_amd.train.calibration import (VectorScaling, lbfgs_minimize, matrix_logits, matrix_z, nll_grid_numpy, nll_matrix_numpy,
                                                nll_vector_numpy, odir_penalty, scale_logits, temper_logits)
from bayesnn_fpga_amd.train.uncertainty import decompose_ensemble_logits
from tests.helpers import build_seeded

KW = dict(dropout_exit=True, dropout="block", dropout_p=0.25, out_dim=10)
NEW = ("bmi_engine_set_matrix_scaling", "bmi_ensemble_moments_matrix", "bmi_nll_matrix_scratch_bytes", "bmi_nll_matrix_scaling_grad")
CS = (10, 37, 100)


def _coeffs(E, C_, seed=0):
    """The issue's test coefficients: diagonal in [0.4, 2.2], bias in [-1, 1], off-diagonal U(-1, 1) * 0.3 / sqrt(C), not symmetric."""
    rng = np.random.default_rng(200 + seed)
    M = rng.uniform(-1.0, 1.0, (E, C_, C_)) * 0.3 / np.sqrt(C_)
    M[:, np.arange(C_), np.arange(C_)] = rng.uniform(0.4, 2.2, (E, C_))
    return M.astype(np.float32), rng.uniform(-1.0, 1.0, (E, C_)).astype(np.float32)


def _problem(C_, T=4, E=2, B=8, seed=0, scale=4.0):
    rng = np.random.default_rng(seed + C_)
    logits = (rng.standard_normal((T, E, B, C_)) * scale).astype(np.float32)
    return logits, rng.integers(0, C_, B)


def test_check_matrix_scaling():
    M, b = check_matrix_scaling(np.eye(10) * 2, None, 4, 10)
    assert M.shape == (4, 10, 10) and b.shape == (4, 10) and M.dtype == b.dtype == np.float32 and M.flags.c_contiguous
    assert np.array_equal(M, np.broadcast_to(np.eye(10, dtype=np.float32) * 2, (4, 10, 10))) and not b.any()
    M, b = check_matrix_scaling(torch.full((4, 10, 10), -2.0), np.ones(10), 4, 10)       # no sign constraint
    assert (M == -2).all() and (b == 1).all() and b.shape == (4, 10)
    M, b = check_matrix_scaling(np.ones((10, 10)), np.arange(40).reshape(4, 10), 4, 10)
    assert np.array_equal(b, np.arange(40, dtype=np.float32).reshape(4, 10))
    assert check_matrix_scaling(None, None, 4, 10) == (None, None)
    for bad in (np.ones(10), np.ones((4, 10)), np.ones((3, 10, 10)), np.ones((4, 10, 9)), np.ones((4, 10, 10, 1)), 1.0, np.ones((10, 4, 10))):
        with pytest.raises(ValueError):
            check_matrix_scaling(bad, None, 4, 10)
    for bad in (np.ones(9), np.ones((3, 10)), np.ones((10, 10)), 1.0):
        with pytest.raises(ValueError):
            check_matrix_scaling(np.eye(10), bad, 4, 10)
    for v in (np.nan, np.inf, -np.inf, 1e39):
        bad = np.ones((4, 10, 10))
        bad[2, 3, 4] = v
        with pytest.raises(ValueError):
            check_matrix_scaling(bad, None, 4, 10)
        bad = np.ones((4, 10))
        bad[1, 2] = v
        with pytest.raises(ValueError):
            check_matrix_scaling(np.eye(10), bad, 4, 10)
    with pytest.raises(ValueError):
        check_matrix_scaling(None, np.ones(10), 4, 10)


def test_model_setters_exclude_each_other_in_every_order_survive_pickling_and_drop_engines():
    m = build_seeded(ResNet18MCEarlyExit, KW)
    assert m.exit_matrix_scaling is None
    maps = {"temperature": (m.set_exit_temperature, ([0.5, 1.0, 2.0, 4.0],), lambda: m.exit_temperature),
            "vector": (m.set_exit_vector_scaling, (np.linspace(0.5, 2.0, 10),), lambda: m.exit_vector_scaling),
            "matrix": (m.set_exit_matrix_scaling, (np.eye(10) + 0.1, np.linspace(-1, 1, 10)), lambda: m.exit_matrix_scaling)}
    for first in maps:
        for second in maps:
            if first == second:
                continue
            set1, args1, get1 = maps[first]
            set2, args2, get2 = maps[second]
            set1(*args1)
            kept = get1()
            with pytest.raises(ValueError):
                set2(*args2)
            assert get2() is None and get1() is kept, (first, second)
            set2(None)                                                          # clearing is always allowed
            set1(None)
            assert get1() is None
            set2(*args2)                                                        # and after clearing the other map is accepted
            assert get2() is not None
            set2(None)
    m._engines["stale"] = object()
    m.set_exit_matrix_scaling(np.eye(10) * 1.5, np.linspace(-1, 1, 40).reshape(4, 10))
    M, b = m.exit_matrix_scaling
    assert m._engines == {} and type(M) is np.ndarray and M.dtype == b.dtype == np.float32 and M.shape == (4, 10, 10) and b.shape == (4, 10)
    for m2 in (pickle.loads(pickle.dumps(m)), copy.deepcopy(m)):
        M2, b2 = m2.exit_matrix_scaling
        assert type(M2) is np.ndarray and np.array_equal(M2, M) and np.array_equal(b2, b) and m2._engines == {}
    m._engines["stale"] = object()
    m.set_exit_matrix_scaling(None)
    assert m.exit_matrix_scaling is None and m._engines == {}


def test_lib_declares_the_entry_points_and_the_abi_version_stays():
    for name in NEW:
        assert name in _lib.EXPORTS
        assert hasattr(_lib.lib(), name)
    assert _lib.ABI_VERSION == 600 and _lib.lib().bmi_version() == 600
    assert (_lib.NLL_MAT_SLAB, _lib.NLL_MAT_ROWS) == (3456, 64)


def test_c_abi_validation():
    """Null handles, wrong counts, the mutual exclusion of the three maps in both directions, null pointers and unsupported shapes: decided
    on the host, before any launch (the pointers are never dereferenced)."""
    g = CompiledGraph(build_seeded(ResNet18MCEarlyExit, KW), "cpu", 4)
    lib, fake = g.lib, C.c_void_p(4096)
    INVALID, UNSUPPORTED, NOMEM, OK = -22, -95, -12, _lib.BMI_OK
    assert lib.bmi_engine_set_matrix_scaling(None, fake, fake, 4, 10) == INVALID
    assert lib.bmi_engine_set_matrix_scaling(g.handle, fake, None, 4, 10) == INVALID
    for E, Cd in ((3, 10), (5, 10), (4, 9), (4, 100), (0, 0)):
        assert lib.bmi_engine_set_matrix_scaling(g.handle, fake, fake, E, Cd) == INVALID
    assert lib.bmi_engine_set_matrix_scaling(g.handle, fake, fake, 4, 10) == OK
    tau = (C.c_float * 4)(0.5, 1.0, 2.0, 4.0)
    ones = (C.c_float * 4)(1.0, 1.0, 1.0, 1.0)
    assert lib.bmi_engine_set_temperature(g.handle, tau, 4) == INVALID           # a matrix is set
    assert lib.bmi_engine_set_vector_scaling(g.handle, fake, fake, 4, 10) == INVALID
    assert lib.bmi_engine_set_temperature(g.handle, ones, 4) == OK               # all ones is off
    assert lib.bmi_engine_set_temperature(g.handle, None, 0) == OK
    assert lib.bmi_engine_set_vector_scaling(g.handle, None, None, 0, 0) == OK   # clearing is always allowed
    assert lib.bmi_engine_set_matrix_scaling(g.handle, None, None, 0, 0) == OK
    assert lib.bmi_engine_set_temperature(g.handle, tau, 4) == OK
    assert lib.bmi_engine_set_matrix_scaling(g.handle, fake, fake, 4, 10) == INVALID       # a temperature is in force
    assert lib.bmi_engine_set_matrix_scaling(g.handle, None, None, 0, 0) == OK
    assert lib.bmi_engine_set_temperature(g.handle, None, 0) == OK
    assert lib.bmi_engine_set_vector_scaling(g.handle, fake, fake, 4, 10) == OK
    assert lib.bmi_engine_set_matrix_scaling(g.handle, fake, fake, 4, 10) == INVALID       # a vector scaling is in force
    assert lib.bmi_engine_set_vector_scaling(g.handle, None, None, 0, 0) == OK
    assert lib.bmi_engine_set_matrix_scaling(g.handle, fake, fake, 4, 10) == OK
    assert lib.bmi_engine_set_matrix_scaling(g.handle, None, None, 0, 0) == OK
    # the stand-alone ensemble entry
    assert lib.bmi_ensemble_moments_matrix(None, 1, 1, 1, 1, fake, fake, None, fake, fake, fake, None) == INVALID
    assert lib.bmi_ensemble_moments_matrix(fake, 1, 1, 1, 1, None, fake, None, fake, fake, fake, None) == INVALID
    assert lib.bmi_ensemble_moments_matrix(fake, 1, 1, 1, 1, fake, None, None, fake, fake, fake, None) == INVALID
    assert lib.bmi_ensemble_moments_matrix(fake, 1, 1, 1, 1, fake, fake, None, None, fake, fake, None) == INVALID
    assert lib.bmi_ensemble_moments_matrix(fake, 0, 1, 1, 1, fake, fake, None, fake, fake, fake, None) == INVALID
    assert lib.bmi_ensemble_moments_matrix(fake, 2, 33, 2, 10, fake, fake, None, fake, fake, fake, None) == UNSUPPORTED
    assert lib.bmi_ensemble_moments_matrix(fake, 2, 2, 2, 129, fake, fake, fake, fake, fake, fake, None) == UNSUPPORTED
    # the fit entry
    assert lib.bmi_nll_matrix_scratch_bytes(4, 250, 100) == 4 * 250 * 10101 * 8
    assert lib.bmi_nll_matrix_scratch_bytes(0, 250, 100) == 0 and lib.bmi_nll_matrix_scratch_bytes(4, 250, 0) == 0
    ok = [fake, 10, 4, 7, 10, fake, fake, fake, fake, fake, fake, fake, 4 * 7 * 111 * 8, None]
    for i in (0, 5, 6, 7, 8, 9, 10, 11):
        args = list(ok)
        args[i] = None
        assert lib.bmi_nll_matrix_scaling_grad(*args) == INVALID, i
    for i in (1, 2, 3, 4):
        args = list(ok)
        args[i] = 0
        assert lib.bmi_nll_matrix_scaling_grad(*args) == INVALID, i
    args = list(ok)
    args[12] -= 1
    assert lib.bmi_nll_matrix_scaling_grad(*args) == NOMEM
    args = list(ok)
    args[4], args[12] = 129, 4 * 7 * (129 * 129 + 130) * 8
    assert lib.bmi_nll_matrix_scaling_grad(*args) == UNSUPPORTED
    args = list(ok)
    args[2], args[12] = 65536, 65536 * 7 * 111 * 8
    assert lib.bmi_nll_matrix_scaling_grad(*args) == UNSUPPORTED


@pytest.mark.parametrize("C_", CS)
def test_a_diagonal_matrix_is_vector_scaling_bit_for_bit(C_):
    """matrix_logits with diag(a) and bias b is array_equal to scale_logits(a, b): the off-diagonal products are +-0 and
    fl(fl(a l_c) + b) is vector scaling's number.  The ensemble restatement agrees the same way."""
    logits = _problem(C_, T=5, E=3, B=4)[0]
    rng = np.random.default_rng(C_)
    a, b = rng.uniform(0.4, 2.2, (3, C_)).astype(np.float32), rng.uniform(-1, 1, (3, C_)).astype(np.float32)
    M = np.zeros((3, C_, C_), np.float32)
    M[:, np.arange(C_), np.arange(C_)] = a
    for got, want in zip(matrix_logits(logits, M, b), scale_logits(logits, a, b)):
        assert np.array_equal(got, want)
    r, w = decompose_ensemble_logits(logits, matrix=M, bias=b), decompose_ensemble_logits(logits, scale=a, bias=b)
    assert all(np.array_equal(r[k], w[k]) for k in w)
    with pytest.raises(ValueError):
        decompose_ensemble_logits(logits, matrix=M, scale=a)
    with pytest.raises(ValueError):
        decompose_ensemble_logits(logits, 2.0, matrix=M)


@pytest.mark.parametrize("C_", CS)
def test_a_permutation_matrix_permutes_the_classes_and_is_not_transposed(C_):
    """z_c = l_pi(c) for M[c][pi(c)] = 1 (row = OUTPUT class): the mean of class c is the unscaled restatement's mean of class pi(c)."""
    logits = _problem(C_, T=5, E=2, B=4)[0]
    pi = np.random.default_rng(C_).permutation(C_)
    assert not np.array_equal(pi, np.argsort(pi))            # (not an involution: a transposed matrix would be caught)
    M = np.zeros((C_, C_), np.float32)
    M[np.arange(C_), pi] = 1.0
    assert np.array_equal(matrix_z(logits, M), logits[..., pi])
    mean, var = matrix_logits(logits, M)
    mean0, var0 = temper_logits(logits, 1.0)
    np.testing.assert_allclose(mean, mean0[..., pi], rtol=0, atol=1e-15)
    np.testing.assert_allclose(var, var0[..., pi], rtol=0, atol=1e-15)


@pytest.mark.parametrize("C_", CS)
def test_nll_matrix_numpy_against_central_differences_the_diagonal_anchor_and_the_gauge(C_):
    """10 random entries of (M, b) per C against central differences of the restatement's own value, step 1e-6, within 1e-7 absolute on
    logits of scale 4; on a diagonal matrix value and gradient are nll_vector_numpy's exactly; the columns of g_matrix and g_bias sum to 0
    to 1e-12 * n."""
    logits, labels = _problem(C_)
    E, n = logits.shape[1], logits.shape[2]
    M, b = (v.astype(np.float64) for v in _coeffs(E, C_))
    f, gM, gb = nll_matrix_numpy(logits, labels, M, b)
    assert f.shape == (E,) and gM.shape == (E, C_, C_) and gb.shape == (E, C_)
    rng, h, worst = np.random.default_rng(C_ + 1), 1e-6, 0.0
    for k in range(10):
        Mp, Mm, bp, bm = M.copy(), M.copy(), b.copy(), b.copy()
        if k < 8:
            c, j = (int(v) for v in rng.integers(0, C_, 2))
            Mp[:, c, j] += h                     # (the exits are independent problems: one perturbation serves all of them)
            Mm[:, c, j] -= h
            want = gM[:, c, j]
        else:
            c = int(rng.integers(0, C_))
            bp[:, c] += h
            bm[:, c] -= h
            want = gb[:, c]
        fd = (nll_matrix_numpy(logits, labels, Mp, bp)[0] - nll_matrix_numpy(logits, labels, Mm, bm)[0]) / (2 * h)
        worst = max(worst, float(np.abs(fd - want).max()))
    print(f"C {C_}: largest absolute error against central differences {worst:.2e}")
    assert worst <= 1e-7
    assert np.abs(gM.sum(1)).max() <= 1e-12 * n and np.abs(gb.sum(1)).max() <= 1e-12 * n
    a = M[:, np.arange(C_), np.arange(C_)]
    D = np.zeros_like(M)
    D[:, np.arange(C_), np.arange(C_)] = a
    fv, ga, gbv = nll_vector_numpy(logits, labels, a, b)
    fd_, gD, gbd = nll_matrix_numpy(logits, labels, D, b)
    assert np.array_equal(fd_, fv) and np.array_equal(gbd, gbv) and np.array_equal(gD[:, np.arange(C_), np.arange(C_)], ga)


def test_odir_penalty_against_central_differences_and_zero_on_a_diagonal():
    E, C_, n = 2, 7, 48
    rng = np.random.default_rng(5)
    M, b = rng.standard_normal((E, C_, C_)), rng.standard_normal((E, C_))
    v, gM, gb = odir_penalty(M, b, n, 0.7, 0.3)
    off = M * (1 - np.eye(C_))
    np.testing.assert_allclose(v, n * (0.7 / (C_ * (C_ - 1)) * (off ** 2).sum((1, 2)) + 0.3 / C_ * (b ** 2).sum(1)), rtol=1e-14)
    h = 1e-6
    for c, j in ((0, 0), (1, 4), (6, 2)):
        Mp, Mm = M.copy(), M.copy()
        Mp[:, c, j] += h
        Mm[:, c, j] -= h
        np.testing.assert_allclose((odir_penalty(Mp, b, n, 0.7, 0.3)[0] - odir_penalty(Mm, b, n, 0.7, 0.3)[0]) / (2 * h), gM[:, c, j], rtol=0, atol=1e-7)
    bp, bm = b.copy(), b.copy()
    bp[:, 3] += h
    bm[:, 3] -= h
    np.testing.assert_allclose((odir_penalty(M, bp, n, 0.7, 0.3)[0] - odir_penalty(M, bm, n, 0.7, 0.3)[0]) / (2 * h), gb[:, 3], rtol=0, atol=1e-7)
    assert not gM[:, np.arange(C_), np.arange(C_)].any()
    D = np.zeros((E, C_, C_))
    D[:, np.arange(C_), np.arange(C_)] = rng.uniform(0.4, 2.2, (E, C_))
    v, gM, gb = odir_penalty(D, b, n, 3.0, 0.0)
    assert not v.any() and not gM.any() and not gb.any()
    v, gM, gb = odir_penalty(None, b, n, 0.0, 0.3)              # VectorScaling's bias term
    assert gM is None and np.array_equal(v, odir_penalty(D, b, n, 0.0, 0.3)[0])


def _banded_teacher_problem():
    """C = 10, 48 images, T = 10, two exits; labels drawn from softmax(M* mean logits) with a banded, non-diagonal M*."""
    C_, N, T, E = 10, 48, 10, 2
    rng = np.random.default_rng(11)
    base = rng.standard_normal((1, E, N, C_)) * 3.0
    logits = (base + rng.standard_normal((T, E, N, C_)) * 0.7).astype(np.float32)
    Ms = np.eye(C_) * 1.5
    for c in range(C_):
        Ms[c, (c + 1) % C_] = 0.9
        Ms[c, (c - 1) % C_] = -0.4
    z = logits.mean(0)[-1].astype(np.float64) @ Ms.T
    p = np.exp(z - z.max(-1, keepdims=True))
    labels = np.array([rng.choice(C_, p=q / q.sum()) for q in p])
    return logits, labels


def test_numpy_fit_on_the_banded_teacher_lowers_the_vector_fits_nll_and_the_penalty_shrinks_the_off_diagonal():
    logits, labels = _banded_teacher_problem()
    T, E, N, C_ = logits.shape

    def vec(x):
        f, ga, gb = nll_vector_numpy(logits, labels, x[:, :C_], x[:, C_:])
        return f, np.concatenate([ga, gb], axis=1)
    v = lbfgs_minimize(vec, np.concatenate([np.ones((E, C_)), np.zeros((E, C_))], axis=1), max_iter=60)
    x0 = np.zeros((E, C_ * C_ + C_))
    D = np.zeros((E, C_, C_))
    D[:, np.arange(C_), np.arange(C_)] = v["x"][:, :C_]
    x0[:, :C_ * C_], x0[:, C_ * C_:] = D.reshape(E, -1), v["x"][:, C_:]
    rms = []
    for lam in (0.0, 1.0, 100.0):
        def obj(x):
            M, b = x[:, :C_ * C_].reshape(E, C_, C_), x[:, C_ * C_:]
            f, gM, gb = nll_matrix_numpy(logits, labels, M, b)
            pv, pM, pb = odir_penalty(M, b, N, lam, 0.0)
            return f + pv, np.concatenate([(gM + pM).reshape(E, -1), gb + pb], axis=1)
        r = lbfgs_minimize(obj, x0, max_iter=60)
        M, b = r["x"][:, :C_ * C_].reshape(E, C_, C_), r["x"][:, C_ * C_:]
        after = nll_matrix_numpy(logits, labels, M, b)[0]
        off = M * (1 - np.eye(C_))
        rms.append(float(np.sqrt((off ** 2).sum() / (E * C_ * (C_ - 1)))))
        print(f"off_diag_l2 {lam}: nll {v['f']} -> {after}, off-diagonal rms {rms[-1]:.3g}")
        assert (after <= v["f"]).all(), (lam, after, v["f"])
    assert rms[0] > rms[1] > rms[2], rms


class _HostEngine:
    """The two device objectives VectorScaling.fit calls, through their numpy restatements."""

    def nll_grid(self, logits, y, grid, out=None):
        r = torch.from_numpy(nll_grid_numpy(logits.numpy(), y.numpy(), grid.numpy()))
        return r if out is None else out + r

    def nll_vector_grad(self, logits, y, a, b, out=None):
        r = tuple(torch.from_numpy(v) for v in nll_vector_numpy(logits.numpy(), y.numpy(), a.numpy(), b.numpy()))
        return r if out is None else tuple(o + v for o, v in zip(out, r))


class _HostVectorScaling(VectorScaling):
    def __init__(self, model, batches):
        self.model, self.device, self.result, self._batches = model, torch.device("cpu"), None, batches

    def collect(self):
        self._engine = _HostEngine()
        return self._batches


def test_vector_scaling_with_bias_l2_zero_never_evaluates_the_penalty(monkeypatch):
    m = build_seeded(ResNet18MCEarlyExit, KW)
    logits, labels = _problem(10, T=3, E=4, B=12, scale=2.0)
    batches = [(torch.from_numpy(logits[:, :, :6].copy()), torch.from_numpy(labels[:6].astype(np.int32))),
               (torch.from_numpy(logits[:, :, 6:].copy()), torch.from_numpy(labels[6:].astype(np.int32)))]
    calls = []
    real = calibration.odir_penalty
    monkeypatch.setattr(calibration, "odir_penalty", lambda *a, **k: calls.append(1) or real(*a, **k))
    r0 = _HostVectorScaling(m, batches).fit(max_iter=8)
    assert not calls and "penalty" not in r0
    r00 = _HostVectorScaling(m, batches).fit(max_iter=8, bias_l2=0.0)
    assert not calls and all(np.array_equal(r0[k], r00[k]) for k in r0)
    r1 = _HostVectorScaling(m, batches).fit(max_iter=8, bias_l2=5.0)
    assert calls and r1["penalty"].shape == (4,) and (r1["penalty"] >= 0).all()
    assert (np.abs(r1["bias"]).sum(1) < np.abs(r0["bias"]).sum(1)).all()
