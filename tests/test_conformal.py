"""-m gpu: conformal prediction sets on the device (bmi_conformal_scores / bmi_conformal_quantile / bmi_conformal_sets, the MCDEngine methods,
ConformalAnalysis) against the plain reference of tests/test_conformal_host.py, bit for bit in every output; the spare record columns stay
as filled, a refused call writes nothing, and the walk over the seeded ResNet-18 equals ``conformal_numpy`` on its own T-mean arrays."""
import ctypes as C

import numpy as np
import pytest
import torch

from bayesnn_fpga_amd import _lib
from bayesnn_fpga_amd.models.resnet18.resnet18 import ResNet18MCEarlyExit
from bayesnn_fpga_amd.synthetic import synthetic_images, synthetic_labels, synthetic_weights_
from bayesnn_fpga_amd.train import ConformalAnalysis
from bayesnn_fpga_amd.train.conformal import conformal_metrics, conformal_numpy
from bayesnn_fpga_amd.train.reliability import classwise_numpy
from tests.gpu_helpers import ptr, stream
from tests.helpers import build_seeded
from tests.test_conformal_host import COVERAGE, IDS, METHODS, SHAPES, expected, make_inputs

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SPARE, FILL = 3, -7                          # record columns beyond N, and what every output is filled with
L = len(COVERAGE)
TABLES = ("valid", "covered", "size_sum", "size_hist", "cov_hist", "class_n", "class_cov")
KW = dict(dropout_exit=True, dropout="block", dropout_p=0.25, out_dim=10)


def filled(shape, dtype):
    return torch.full(shape, FILL % 256 if dtype == torch.uint8 else FILL, dtype=dtype, device=DEV)


def untouched(t):
    return bool((t == (FILL % 256 if t.dtype == torch.uint8 else FILL)).all())


def outputs(R, Cd, cap):
    """every output of the three calls, filled"""
    t = dict(valid=(R,), covered=(R, L), size_sum=(R, L), size_hist=(R, L, Cd + 1), cov_hist=(R, L, Cd + 1), class_n=(R, Cd), class_cov=(R, L, Cd))
    return dict(score_keys=filled((R, cap), torch.int32), qhat=filled((R, L), torch.int32), n_valid=filled((R,), torch.int64),
                set_size=filled((R, L, cap), torch.uint8), members=filled((R, L, (Cd + 31) // 32, cap), torch.int32),
                **{k: filled(s, torch.int64) for k, s in t.items()})


def calls(pkeys, labels, R, Cd, N, cap, method, o, members=True, levels=L, run=(0, 1, 2)):
    """the three calls (or those of ``run``) in turn -> their return codes"""
    lib, (name, k_reg, lam) = _lib.lib(), method
    code, lam_fix = _lib.CONFORMAL_METHODS[name], int(lam * 2 ** 30)
    three = [lambda: lib.bmi_conformal_scores(ptr(pkeys), ptr(labels), R, Cd, N, cap, code, k_reg, lam_fix, ptr(o["score_keys"]), stream()),
             lambda: lib.bmi_conformal_quantile(ptr(o["score_keys"]), R, N, cap, (C.c_double * 9)(*COVERAGE), levels, ptr(o["qhat"]),
                                                ptr(o["n_valid"]), stream()),
             lambda: lib.bmi_conformal_sets(ptr(pkeys), ptr(labels), R, Cd, N, cap, code, k_reg, lam_fix, ptr(o["qhat"]), levels, ptr(o["set_size"]),
                                            ptr(o["members"]) if members else None, *(ptr(o[k]) for k in TABLES), stream())]
    rcs = [three[i]() for i in run]
    torch.cuda.synchronize()
    return rcs


def host(t):
    a = t.cpu().numpy()
    return a.view(np.uint32) if a.dtype == np.int32 else a


@pytest.mark.parametrize("shape", SHAPES, **IDS)
def test_kernels_equal_the_plain_reference(shape):
    """Records written by bmi_classwise_record (a NaN row and a bad label among them) into N + 3 columns; per method the three calls"""
    Cd, E, N = shape
    p, y, t = make_inputs(*shape)
    R, cap = 2 * E, N + SPARE
    pkeys, labels = filled((R, Cd, cap), torch.int32), filled((cap,), torch.int32)
    mean, yd = torch.from_numpy(p).to(DEV), torch.from_numpy(y.astype(np.int32)).to(DEV)
    assert _lib.lib().bmi_classwise_record(ptr(mean), E, N, Cd, ptr(yd), 0, cap, ptr(pkeys), ptr(labels), None, stream()) == 0
    assert np.array_equal(host(pkeys)[:, :, :N], t["pkeys"]) and np.array_equal(labels.cpu().numpy()[:N], t["labels"])
    for method in METHODS:
        want = expected(shape, method)[2]
        for members in (True, False):
            o = outputs(R, Cd, cap)
            assert calls(pkeys, labels, R, Cd, N, cap, method, o, members) == [0, 0, 0], method
            for name in ("score_keys", "set_size", "members"):
                a = host(o[name])
                if name == "members" and not members:
                    assert untouched(o[name])
                    continue
                assert np.array_equal(a[..., :N], want[name]), (method, name)
                assert untouched(o[name][..., N:]), (method, name)                      # the spare columns: as filled
            for name in ("qhat", "n_valid") + TABLES:
                assert np.array_equal(host(o[name]), want[name]), (method, name)
    assert untouched(pkeys[:, :, N:]) and untouched(labels[N:])


def test_a_refused_call_writes_nothing():
    """Every refused call returns its code and leaves every canary-filled output as filled; no buffer is refilled in between"""
    R, Cd, N, cap = 2, 10, 5, 8
    pkeys, labels = torch.zeros(R, 129, cap, dtype=torch.int32, device=DEV), torch.zeros(cap, dtype=torch.int32, device=DEV)
    o = outputs(R, 129, cap)
    aps = METHODS[1]
    for what, rcs, want in (
            ("C = 129 (UNSUPPORTED)", lambda: calls(pkeys, labels, R, 129, N, cap, aps, o, run=(0, 2)), [-95, -95]),
            ("R = 65 (UNSUPPORTED)", lambda: calls(pkeys, labels, 65, Cd, N, cap, aps, o), [-95, -95, -95]),
            ("L = 9", lambda: calls(pkeys, labels, R, Cd, N, cap, aps, o, levels=9, run=(1, 2)), [-22, -22]),
            ("L = 0", lambda: calls(pkeys, labels, R, Cd, N, cap, aps, o, levels=0, run=(1, 2)), [-22, -22]),
            ("N > N_cap", lambda: calls(pkeys, labels, R, Cd, cap + 1, cap, aps, o), [-22, -22, -22]),
            ("null records", lambda: calls(None, labels, R, Cd, N, cap, aps, o, run=(0, 2)), [-22, -22]),
            ("null outputs", lambda: calls(pkeys, labels, R, Cd, N, cap, aps, dict(o, score_keys=None, valid=None)), [-22, -22, -22]),
            ("null qhat", lambda: calls(pkeys, labels, R, Cd, N, cap, aps, dict(o, qhat=None), run=(1, 2)), [-22, -22]),
            ("k_reg < 0", lambda: calls(pkeys, labels, R, Cd, N, cap, ("raps", -1, 0.5), o, run=(0, 2)), [-22, -22])):
        assert rcs() == want, what
        assert all(untouched(v) for v in o.values()), what


def test_conformal_analysis_against_the_restatement_on_its_own_means():
    """The seeded ResNet-18, T = 4: fit on 2 batches of 8, evaluate on 2 more, predict one batch; quantiles, sets and tables equal
    conformal_numpy on classwise_numpy of the analysis's own T-mean arrays"""
    m = synthetic_weights_(build_seeded(ResNet18MCEarlyExit, KW), 0).to(DEV).eval()
    B, cov = 8, (0.5, 0.8)
    x, y = synthetic_images(4 * B, seed=3), synthetic_labels(4 * B, 10, seed=4)
    loaders = [[(x[i * B:(i + 1) * B], y[i * B:(i + 1) * B]) for i in pair] for pair in ((0, 1), (2, 3))]
    for method in (("aps", 0, 0.0), ("raps", 2, 0.05)):
        ca = ConformalAnalysis(m, gpu=0, mc_passes=4, seed=11, method=method[0], k_reg=method[1], lam=method[2], coverage=cov, keep_mean=True)
        with pytest.raises(RuntimeError):
            ca.predict(x[:B])
        ca.fit(loaders[0])
        ev = ca.evaluate(loaders[1])
        fit = classwise_numpy(ca.fit_mean, ca.fit_labels)
        want_fit = conformal_numpy(fit["pkeys"], fit["labels"], *method, cov)
        assert np.array_equal(host(ca.scores), want_fit["score_keys"]) and np.array_equal(host(ca.qhat), want_fit["qhat"])
        assert np.array_equal(ca.n_valid.cpu().numpy(), want_fit["n_valid"]) and ca.n_valid.tolist() == [2 * B] * 8
        test = classwise_numpy(ev["mean"], ev["labels"])
        want = conformal_numpy(test["pkeys"], test["labels"], *method, cov, qhat=want_fit["qhat"])
        for name in ("set_size", "members") + TABLES:
            assert np.array_equal(host(ev[name])[..., :2 * B] if name in ("set_size", "members") else host(ev[name]), want[name]), name
        wm = conformal_metrics(want)
        assert all(np.array_equal(ev["metrics"][k], wm[k], equal_nan=True) for k in wm)
        pr = ca.predict(x[:B].to(DEV))
        assert tuple(pr["set_size"].shape) == (8, 2, B) and tuple(pr["members"].shape) == (8, 2, 1, B) and "covered" not in pr
        sizes = np.array([[[bin(int(w)).count("1") for w in lv[0]] for lv in row] for row in host(pr["members"])])
        assert np.array_equal(sizes, pr["set_size"].cpu().numpy()) and (sizes <= 10).all()
