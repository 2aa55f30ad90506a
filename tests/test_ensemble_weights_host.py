"""Weighted exit ensembles, CPU side: the host restatement (decompose_ensemble_logits(weights=)) against direct torch float64 arithmetic
and its two bit-for-bit identities (uniform power-of-two rows, one-hot rows), the validation and expansion of the accepted forms (model,
C ABI), the EM fit of one row (monotone, KKT), and the loader-level fit on the CPU oracle's means."""
import ctypes as C
import pickle

import numpy as np
import pytest
import torch

from bayesnn_fpga_amd import _lib
from bayesnn_fpga_amd.engine import CompiledGraph, check_ensemble_weights
from bayesnn_fpga_amd.models.resnet18.resnet18 import ResNet18MCEarlyExit
from bayesnn_fpga_amd.train.calibration import EnsembleWeights, mixture_nll, mixture_weights_em
from bayesnn_fpga_amd.train.uncertainty import decompose_ensemble_logits, weighted_exit_ensembles
from tests.helpers import build_seeded

KW = dict(dropout_exit=True, dropout="block", dropout_p=0.25, out_dim=10)
NAMES = ("mean", "var", "pred_entropy", "exp_entropy", "mutual_info")


def _logits(shape=(19, 4, 3, 100), scale=3.0, seed=5):
    return (np.random.default_rng(seed).standard_normal(shape) * scale).astype(np.float32)


def _simplex_rows(E, seed, zeros=False):
    rng = np.random.default_rng(seed)
    W = np.zeros((E, E))
    for e in range(E):
        w = rng.random(e + 1) + 0.05
        if zeros and e >= 1:
            w[rng.integers(0, e + 1)] = 0.0          # an exact zero in the row (never the whole row: e + 1 >= 2 entries)
        W[e, :e + 1] = w / w.sum()
    return check_ensemble_weights(W, E)


def test_lib_declares_the_entry_points_and_the_abi_version_stays():
    for name in ("bmi_engine_set_ensemble_weights", "bmi_ensemble_moments_weighted"):
        assert name in _lib.EXPORTS
        assert hasattr(_lib.lib(), name)
    assert _lib.ABI_VERSION == 600 and _lib.lib().bmi_version() == 600          # additive, like the temperature entry points


def _torch_restatement(logits, W, tau=None):
    """softmax -> weighted sum over exits -> moments over T, float64 torch (matmul-free, but in no particular order)."""
    l = torch.from_numpy(np.asarray(logits, dtype=np.float32))
    T, E = l.shape[:2]
    if tau is not None:
        inv = torch.from_numpy((1.0 / np.asarray(tau, dtype=np.float32).astype(np.float64)).astype(np.float32))
        l = l * inv.view(1, E, 1, 1)
    p = torch.softmax(l.double(), dim=-1)                                       # [T, E, B, C]
    q = torch.einsum("ei,tibc->tebc", torch.from_numpy(np.asarray(W)), p)
    mean = q.mean(0)
    var = (q * q).mean(0) - mean * mean
    ent = lambda a: -(torch.where(a > 0, a * torch.log(torch.where(a > 0, a, torch.ones_like(a))), torch.zeros_like(a))).sum(-1)
    pe, ee = ent(mean), ent(q).mean(0)
    return {k: v.numpy() for k, v in dict(mean=mean, var=var.clamp_min(0), pred_entropy=pe, exp_entropy=ee,
                                          mutual_info=(pe - ee).clamp_min(0)).items()}


@pytest.mark.parametrize("shape", [(19, 4, 3, 100), (7, 5, 2, 128), (5, 1, 2, 1), (9, 3, 2, 33)], ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("zeros", [False, True], ids=["simplex", "with_zeros"])
def test_host_restatement_against_direct_torch_float64(shape, zeros):
    """1e-13 absolute on mean / var (values in [0, 1], a handful of float64 roundings apart: the two sides differ in summation order) and
    1e-11 on the entropies (sums of at most 128 terms of size <= 0.37, then a difference)."""
    logits, E = _logits(shape), shape[1]
    W = _simplex_rows(E, seed=shape[0], zeros=zeros)
    for tau in (None, [0.6 + 0.45 * e for e in range(E)]):
        got, ref = decompose_ensemble_logits(logits, tau, weights=W), _torch_restatement(logits, W, tau)
        for k in NAMES:
            tol = 1e-13 if k in ("mean", "var") else 1e-11
            err = float(np.abs(got[k] - ref[k]).max())
            assert err <= tol, f"{shape} tau={tau is not None} {k}: {err:.3e}"
    if E > 1:
        assert np.abs(decompose_ensemble_logits(logits, weights=W)["mean"] - decompose_ensemble_logits(logits)["mean"]).max() > 1e-4


def test_uniform_weights_are_the_equal_mean_bit_for_bit_on_power_of_two_rows():
    """W[e][i] = 1 / (e + 1): on rows 0, 1 and 3 the products w * p are exact scalings by a power of two, which commute with rounding, so
    the weighted sum IS the equal mean's running sum divided once.  Row 2 (1/3 is rounded, and so is every product) agrees to
    T * 4 * 2^-53 on the sums: three products and a sum of three terms, each within 2^-53 of values <= 1, per sample."""
    logits = _logits()
    T = logits.shape[0]
    plain, uni = decompose_ensemble_logits(logits), decompose_ensemble_logits(logits, weights=np.ones(4))
    for e in (0, 1, 3):
        for k in NAMES:
            assert np.array_equal(plain[k][e], uni[k][e]), (e, k)
    # row 2 on the sums themselves, restated here (decompose's mean is this Q1 / T bit for bit)
    z = logits.astype(np.float64)
    z = z - z.max(axis=-1, keepdims=True)
    p = np.exp(z) / np.exp(z).sum(axis=-1, keepdims=True)
    w = check_ensemble_weights(np.ones(4), 4)[2]
    q1_plain, q1_uni = np.zeros(p.shape[2:]), np.zeros(p.shape[2:])
    for t in range(T):
        q1_plain += ((p[t, 0] + p[t, 1]) + p[t, 2]) / 3
        q1_uni += ((0.0 + w[0] * p[t, 0]) + w[1] * p[t, 1]) + w[2] * p[t, 2]
    assert np.array_equal(q1_plain / T, plain["mean"][2]) and np.array_equal(q1_uni / T, uni["mean"][2])
    err = float(np.abs(q1_plain - q1_uni).max())
    print(f"row 2, Q1: {err:.3e}")
    assert err <= T * 4 * 2.0 ** -53


def test_one_hot_rows_are_the_single_exit_slice_bit_for_bit():
    logits = _logits()
    E = logits.shape[1]
    for ks in ([0, 0, 0, 0], [0, 1, 2, 3], [0, 1, 0, 2], [0, 0, 2, 1]):
        W = np.zeros((E, E))
        for e, k in enumerate(ks):
            W[e, k] = 1.0
        got = decompose_ensemble_logits(logits, weights=W)
        for e, k in enumerate(ks):
            ref = decompose_ensemble_logits(logits[:, k:k + 1])
            for n in NAMES:
                assert np.array_equal(got[n][e], ref[n][0]), (ks, e, n)


def test_vector_expansion_and_accepted_forms():
    assert check_ensemble_weights(None, 4) is None
    W = check_ensemble_weights([1.0, 2.0, 3.0, 4.0], 4)
    assert W.dtype == np.float64 and W.shape == (4, 4) and W.flags["C_CONTIGUOUS"]
    want = np.array([[1, 0, 0, 0], [1 / 3, 2 / 3, 0, 0], [1 / 6, 2 / 6, 3 / 6, 0], [0.1, 0.2, 0.3, 0.4]])
    assert np.array_equal(W, want)
    assert np.array_equal(check_ensemble_weights(torch.tensor([1.0, 2.0, 3.0, 4.0]), 4), want)
    assert np.array_equal(check_ensemble_weights(want, 4), want)                # a matrix is taken as given
    assert np.array_equal(check_ensemble_weights([2.0, 0.0, 0.0, 6.0], 4)[3], [0.25, 0, 0, 0.75])     # zeros behind a positive prefix
    assert np.array_equal(check_ensemble_weights([5.0], 1), [[1.0]]) and np.array_equal(check_ensemble_weights([[1.0]], 1), [[1.0]])
    assert np.array_equal(weighted_exit_ensembles(np.arange(8.0).reshape(4, 2), np.eye(4)), np.arange(8.0).reshape(4, 2))


_I4 = np.eye(4)
BAD = {
    "negative": [1.0, -1.0, 1.0, 1.0],
    "nan": [1.0, float("nan"), 1.0, 1.0],
    "inf": [1.0, float("inf"), 1.0, 1.0],
    "zero_prefix": [0.0, 1.0, 1.0, 1.0],
    "wrong_count": [1.0, 1.0, 1.0],
    "wrong_matrix": np.eye(3),
    "three_dims": np.zeros((4, 4, 1)),
    "scalar": 1.0,
    "above_diagonal": np.array([[0.5, 0.5, 0, 0], [0, 1, 0, 0], [0, 0, 1, 0], [0, 0, 0, 1.0]]),
    "row_sum_high": _I4 + np.diag([0, 0, 0, 3e-12]),
    "row_sum_low": _I4 - np.diag([0, 2e-12, 0, 0]),
    "negative_matrix": np.array([[1, 0, 0, 0], [1.5, -0.5, 0, 0], [0, 0, 1, 0], [0, 0, 0, 1.0]]),
    "nan_matrix": np.array([[1, 0, 0, 0], [float("nan"), 1, 0, 0], [0, 0, 1, 0], [0, 0, 0, 1.0]]),
}


@pytest.mark.parametrize("bad", list(BAD), ids=list(BAD))
def test_validation_errors_on_the_host(bad):
    m = build_seeded(ResNet18MCEarlyExit, KW)
    with pytest.raises(ValueError):
        m.set_exit_ensemble_weights(BAD[bad])
    assert m.exit_ensemble_weights is None
    with pytest.raises(ValueError):
        check_ensemble_weights(BAD[bad], 4)
    with pytest.raises(ValueError):
        decompose_ensemble_logits(_logits((2, 4, 1, 3)), weights=BAD[bad])
    assert check_ensemble_weights(_I4 + np.diag([0, 0, 0, 5e-13]), 4) is not None        # inside the 1e-12 band


def test_model_attribute_is_a_plain_array_and_survives_pickling():
    m = build_seeded(ResNet18MCEarlyExit, KW)
    assert m.exit_ensemble_weights is None
    m.set_exit_temperature([0.5, 1.0, 2.5, 4.0])
    m.set_exit_ensemble_weights([1.0, 2.0, 3.0, 4.0])
    W = m.exit_ensemble_weights
    assert type(W) is np.ndarray and W.dtype == np.float64 and W.shape == (4, 4) and m._engines == {}
    m2 = pickle.loads(pickle.dumps(m))
    assert type(m2.exit_ensemble_weights) is np.ndarray and np.array_equal(m2.exit_ensemble_weights, W)
    assert m2.exit_temperature == [0.5, 1.0, 2.5, 4.0]
    m.set_exit_ensemble_weights(None)
    assert m.exit_ensemble_weights is None and m.exit_temperature == [0.5, 1.0, 2.5, 4.0]


def test_c_abi_validation():
    """The handle-level entry validates the handle and the count only (the contents are the Python layer's job); the stand-alone entry
    refuses null pointers and bad counts on the host, before any launch."""
    g = CompiledGraph(build_seeded(ResNet18MCEarlyExit, KW), "cpu", 4)
    lib = g.lib
    fake = C.c_void_p(4096)                    # never dereferenced on the host
    assert lib.bmi_engine_set_ensemble_weights(g.handle, fake, 4) == _lib.BMI_OK
    assert lib.bmi_engine_set_ensemble_weights(g.handle, fake, 3) == -22
    assert lib.bmi_engine_set_ensemble_weights(g.handle, fake, 5) == -22
    assert lib.bmi_engine_set_ensemble_weights(None, fake, 4) == -22
    assert lib.bmi_engine_set_ensemble_weights(g.handle, None, 0) == _lib.BMI_OK
    assert lib.bmi_ensemble_moments_weighted(None, 1, 1, 1, 1, None, fake, fake, fake, fake, None) == -22
    assert lib.bmi_ensemble_moments_weighted(fake, 1, 1, 1, 1, None, None, fake, fake, fake, None) == -22
    assert lib.bmi_ensemble_moments_weighted(fake, 0, 1, 1, 1, None, fake, fake, fake, fake, None) == -22
    assert lib.bmi_ensemble_moments_weighted(fake, 2, 33, 2, 10, None, fake, fake, fake, fake, None) == -95
    assert lib.bmi_ensemble_moments_weighted(fake, 2, 2, 2, 129, None, fake, fake, fake, fake, None) == -95
    bad_tau = (C.c_float * 2)(1.0, 0.0)
    assert lib.bmi_ensemble_moments_weighted(fake, 2, 2, 2, 10, bad_tau, fake, fake, fake, fake, None) == -22


# ---- the EM fit -------------------------------------------------------------------------------------------------------------------------
def _em_table(seed=3, N=2000):
    """[4, N] member likelihoods: two members that are each right where the other is wrong (an interior optimum), a mediocre one, and one
    dominated everywhere by member 0 (its optimal weight is 0)."""
    rng = np.random.default_rng(seed)
    side = rng.random(N) < 0.45
    a0 = np.where(side, rng.uniform(0.5, 0.95, N), rng.uniform(0.01, 0.2, N))
    a2 = np.where(side, rng.uniform(0.01, 0.2, N), rng.uniform(0.5, 0.95, N))
    a3 = rng.uniform(0.2, 0.5, N)
    return np.stack([a0, 0.7 * a0, a2, a3])


def test_em_is_monotone_and_meets_the_kkt_conditions():
    """The NLL of a mixture is convex in its weights, so the KKT conditions are exact: g_i = mean_n(A_i / mix) <= 1 for every member, = 1
    where w_i > 0.  At rtol = 1e-12 the residuals are checked to 1e-4."""
    A = _em_table()
    r = mixture_weights_em(A, rtol=1e-12)
    w = r["w"]
    assert r["converged"] and w.shape == (4,) and (w >= 0).all() and abs(float(w.sum()) - 1) <= 1e-15 * 8
    assert np.all(np.diff(r["trace"]) <= 0), "the NLL must not rise in any iteration"
    assert r["trace"][0] == r["nll_uniform"] == mixture_nll(A, np.full(4, 0.25)) and r["trace"][-1] == r["nll"] == mixture_nll(A, w)
    assert r["nll"] <= r["nll_uniform"]
    g = (A / (w @ A)).mean(axis=1)
    print(f"w = {w}, g - 1 = {g - 1}, iterations = {r['iterations']}, nll {r['nll_uniform']:.3f} -> {r['nll']:.3f}")
    assert np.all(g <= 1 + 1e-4)
    assert np.all(np.abs(g - 1)[w >= 1e-3] <= 1e-4)
    assert w[1] < 1e-6 and (w[[0, 2]] > 0.1).all()        # the dominated member is driven out, the complementary pair shares the weight
    check_ensemble_weights(np.vstack([np.eye(4)[:3], w]), 4)          # a fitted row is an acceptable row
    one = mixture_weights_em(A[:1])
    assert np.array_equal(one["w"], [1.0]) and one["nll"] == one["nll_uniform"]
    for bad in (A[0], -A, np.full((2, 3), np.nan), np.zeros((0, 3))):
        with pytest.raises(ValueError):
            mixture_weights_em(bad)


class _OracleEngine:
    """MCDEngine.predict's ``mean`` from the CPU oracle (what EnsembleWeights reads of an engine)."""

    def __init__(self, oracle):
        self.oracle = oracle

    def predict(self, x, T, seed=0, t_begin=0, cnt0=0):
        from oracle import mcd
        return dict(mean=torch.from_numpy(mcd.mcd_predict(self.oracle, x, T, seed, t_begin=t_begin)["mean"]).double())

    def check_finite(self):
        pass


def test_ensemble_weights_on_the_cpu_oracle(tmp_path, monkeypatch):
    """The loader-level fit with the oracle in the engine's place: its table is mean[e, n, y_n] of the per-batch oracle predictions under
    seed + k, its rows are mixture_weights_em on rows 0..e of that table, apply() stores the matrix on the model, save() writes it."""
    from bayesnn_fpga_amd.synthetic import synthetic_images, synthetic_labels, synthetic_weights_
    from oracle import mcd
    from oracle.resnet18 import ResNet18MCEarlyExit as OracleResNet
    oracle = synthetic_weights_(build_seeded(OracleResNet, KW), 0)
    m = build_seeded(ResNet18MCEarlyExit, KW)

    class OracleEnsembleWeights(EnsembleWeights):
        def _engine_for(self, x):
            return _OracleEngine(oracle)

    B, T, seed = 4, 3, 9
    x, y = synthetic_images(3 * B, seed=3), synthetic_labels(3 * B, 10, seed=4)
    loader = [(x[i * B:(i + 1) * B], y[i * B:(i + 1) * B]) for i in range(3)]
    ew = OracleEnsembleWeights(m, loader, gpu=-1, mc_passes=T, seed=seed)
    with pytest.raises(RuntimeError):
        ew.apply()
    r = ew.fit()
    A = np.concatenate([mcd.mcd_predict(oracle, bx, T, seed + k)["mean"][:, np.arange(B), np.asarray(by)] for k, (bx, by) in enumerate(loader)],
                       axis=1)
    assert np.array_equal(ew.table, A) and r["n"] == 3 * B
    W = r["weights"]
    for e in range(4):
        em = mixture_weights_em(A[:e + 1])
        assert np.array_equal(W[e, :e + 1], em["w"]) and not W[e, e + 1:].any()
        assert r["nll_after"][e] == em["nll"] <= r["nll_uniform"][e] == mixture_nll(A[:e + 1], np.full(e + 1, 1 / (e + 1)))
        assert r["nll_per_exit"][e] == float(-np.log(A[e]).sum())
    assert np.array_equal(W[0], [1, 0, 0, 0]) and r["converged"].all()
    assert np.array_equal(ew.apply(), W) and np.array_equal(m.exit_ensemble_weights, W)
    monkeypatch.chdir(tmp_path)
    f = np.load(ew.save("t"))
    assert np.array_equal(f["weights"], W) and set(f.files) == set(r)
    bad = y.clone()
    bad[5] = 10
    with pytest.raises(ValueError, match="labels"):
        OracleEnsembleWeights(m, [(x, bad)], gpu=-1, mc_passes=T).fit()
