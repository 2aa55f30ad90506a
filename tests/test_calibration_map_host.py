"""The one rule of the calibration maps without a GPU, as a table over the kinds (temperature, vector, matrix): engine.resolve_calibration_map
(every pair refused, a bias alone refused, each kind alone gives its check_* function's arrays), the model setters in all six orders and
through a pickle, train.uncertainty.calibrated_logits against the values recorded before the resolver existed
(tests/golden/calibrated_logits.npz), and the C ABI's return codes for null, conflicting and half-given maps (no call reaches a kernel)."""
import ctypes as C
import itertools
import os
import pickle

import numpy as np
import pytest

from bayesnn_fpga_amd import _lib
from bayesnn_fpga_amd.engine import (CompiledGraph, check_matrix_scaling, check_temperature, check_vector_scaling, resolve_calibration_map)
from bayesnn_fpga_amd.models.resnet18.resnet18 import ResNet18MCEarlyExit
from bayesnn_fpga_amd.train.uncertainty import calibrated_logits
from tests.helpers import build_seeded

KW = dict(dropout_exit=True, dropout="block", dropout_p=0.25, out_dim=10)
E, CD = 4, 10
GOLDEN = os.path.join(os.path.dirname(__file__), "golden", "calibrated_logits.npz")
INVALID, UNSUPPORTED, OK = -22, -95, _lib.BMI_OK

# kind -> the resolver's keyword arguments
GIVEN = {"temperature": dict(tau=[0.5, 1.0, 2.0, 4.0]),
         "vector": dict(scale=np.linspace(0.5, 2.0, CD), bias=np.linspace(-1, 1, E * CD).reshape(E, CD)),
         "matrix": dict(matrix=np.eye(CD) + 0.1, bias=np.linspace(-1, 1, CD))}
KINDS = tuple(GIVEN)


def _resolve(**given):
    return resolve_calibration_map(**given, n_exits=E, out_dim=CD, who="the test")


@pytest.mark.parametrize("kinds", list(itertools.combinations(KINDS, 2)) + [KINDS], ids="+".join)
def test_maps_given_together_are_refused(kinds):
    given = {}
    for k in kinds:
        given.update(GIVEN[k])
    with pytest.raises(ValueError, match="the test"):
        _resolve(**given)


def test_a_bias_alone_is_refused_and_nothing_is_no_map():
    with pytest.raises(ValueError, match="the test"):
        _resolve(bias=np.ones(CD))
    with pytest.raises(ValueError, match="the test"):
        _resolve(tau=2.0, bias=np.ones(CD))
    m = _resolve()
    assert m.kind is None and m.tau is None and m.weight is None and m.bias is None


@pytest.mark.parametrize("kind", KINDS)
def test_each_kind_alone_returns_what_its_check_returns(kind):
    m = _resolve(**GIVEN[kind])
    assert m.kind == kind
    if kind == "temperature":
        assert m.tau == check_temperature(GIVEN[kind]["tau"], E) and m.weight is None and m.bias is None
        assert _resolve(tau=1.5).tau == [1.5] * E
    else:
        check = check_vector_scaling if kind == "vector" else check_matrix_scaling
        first = GIVEN[kind]["scale" if kind == "vector" else "matrix"]
        w, b = check(first, GIVEN[kind]["bias"], E, CD)
        assert m.tau is None and np.array_equal(m.weight, w) and np.array_equal(m.bias, b)
        assert m.weight.dtype == m.bias.dtype == np.float32 and m.weight.flags.c_contiguous and m.weight.shape == w.shape
    for bad in (dict(tau=0.0), dict(tau=[1.0, 2.0]), dict(scale=np.ones(CD + 1)), dict(matrix=np.ones((CD, CD + 1))), dict(scale=np.full(CD, np.inf))):
        with pytest.raises(ValueError):
            _resolve(**bad)


def _model_maps(m):
    return {"temperature": (m.set_exit_temperature, (GIVEN["temperature"]["tau"],), "exit_temperature"),
            "vector": (m.set_exit_vector_scaling, (GIVEN["vector"]["scale"], GIVEN["vector"]["bias"]), "exit_vector_scaling"),
            "matrix": (m.set_exit_matrix_scaling, (GIVEN["matrix"]["matrix"], GIVEN["matrix"]["bias"]), "exit_matrix_scaling")}


@pytest.fixture(scope="module")
def model():
    return build_seeded(ResNet18MCEarlyExit, KW)


@pytest.mark.parametrize("first,second", list(itertools.permutations(KINDS, 2)))
def test_model_setters_exclude_each_other_and_clearing_readmits(model, first, second):
    maps = _model_maps(model)
    (set1, args1, attr1), (set2, args2, attr2) = maps[first], maps[second]
    set1(*args1)
    kept = getattr(model, attr1)
    model._engines["stale"] = object()
    with pytest.raises(ValueError):
        set2(*args2)
    assert getattr(model, attr2) is None and getattr(model, attr1) is kept and "stale" in model._engines      # a refused call changes nothing
    set2(None)                                                              # clearing what is not set is allowed
    assert getattr(model, attr1) is kept
    set1(None)
    assert getattr(model, attr1) is None and model._engines == {}
    set2(*args2)
    assert getattr(model, attr2) is not None
    set2(None)
    assert all(getattr(model, a) is None for _, _, a in maps.values())


@pytest.mark.parametrize("kind", KINDS)
def test_a_pickle_round_trip_keeps_the_four_attributes(model, kind):
    set_, args, attr = _model_maps(model)[kind]
    set_(*args)
    model.set_exit_ensemble_weights([1.0, 2.0, 3.0, 4.0])
    try:
        m2 = pickle.loads(pickle.dumps(model))
        for name in ("exit_temperature", "exit_vector_scaling", "exit_matrix_scaling", "exit_ensemble_weights"):
            old, new = getattr(model, name), getattr(m2, name)
            assert type(new) is type(old)
            if isinstance(old, tuple):
                assert all(type(x) is np.ndarray and x.dtype == y.dtype and np.array_equal(x, y) for x, y in zip(new, old))
            elif isinstance(old, np.ndarray):
                assert new.dtype == np.float64 and np.array_equal(new, old)
            else:
                assert new == old
        assert type(m2.exit_temperature) in (list, type(None)) and m2._engines == {}
        assert "exit_" + {"temperature": "temperature", "vector": "vector_scaling", "matrix": "matrix_scaling"}[kind] in m2.__dict__
    finally:
        set_(None)
        model.set_exit_ensemble_weights(None)


@pytest.mark.parametrize("kind", KINDS + ("none",))
def test_calibrated_logits_are_the_recorded_bits(kind):
    """T = 2, E = 2, B = 3, C = 5: z and W of calibrated_logits as commit 1228f36 (the last before the resolver) returned them for the
    inputs the fixture holds beside them (logits, tau, scale / vbias, matrix / mbias, weights), byte for byte."""
    g = np.load(GOLDEN)
    given = {"none": {}, "temperature": dict(tau=g["tau"]), "vector": dict(scale=g["scale"], bias=g["vbias"]),
             "matrix": dict(matrix=g["matrix"], bias=g["mbias"])}[kind]
    z, W = calibrated_logits(g["logits"], weights=g["weights"], **given)
    assert z.dtype == np.float32 and z.shape == (2, 2, 3, 5) and z.tobytes() == g[f"z_{kind}"].tobytes()
    assert W.dtype == np.float64 and W.tobytes() == g["W"].tobytes()
    assert calibrated_logits(g["logits"], **given)[1] is None
    for bad in (0.0, -1.0, np.nan, [1.0]):                                  # what the engines refuse is refused here too
        with pytest.raises(ValueError):
            calibrated_logits(g["logits"], tau=bad)


def test_c_abi_codes_of_the_map_arguments():
    """bmi_vote_counts, bmi_ensemble_moments* and bmi_engine_set_*: the codes tests/test_votes_host.py, test_vector_scaling_host.py,
    test_matrix_scaling_host.py and test_ensemble_weights_host.py pin, as tables.  The fake device pointers are never dereferenced."""
    g = CompiledGraph(build_seeded(ResNet18MCEarlyExit, KW), "cpu", 4)
    lib, fake = g.lib, C.c_void_p(4096)
    tau, ones = (C.c_float * 33)(*([1.5] * 33)), (C.c_float * 4)(1.0, 1.0, 1.0, 1.0)
    bad_taus = [(C.c_float * E)(1.0, v, 1.0, 1.0) for v in (0.0, -1.0, float("nan"), float("inf"), 1e-45)]

    # bmi_vote_counts(logits, T, E, B, C, tau, scale, bias, matrix, W, V, nonfinite, stream)
    def votes(T=3, E_=E, B=7, Cd=CD, tau=None, scale=None, bias=None, matrix=None, logits=fake, V=fake):
        return lib.bmi_vote_counts(logits, T, E_, B, Cd, tau, scale, bias, matrix, None, V, None, None)

    table = [(dict(logits=None), INVALID), (dict(V=None), INVALID),
             (dict(tau=tau, scale=fake, bias=fake), INVALID), (dict(tau=tau, matrix=fake, bias=fake), INVALID),
             (dict(scale=fake, matrix=fake, bias=fake), INVALID), (dict(bias=fake), INVALID), (dict(scale=fake), INVALID),
             (dict(matrix=fake), INVALID), (dict(tau=tau, bias=fake), INVALID),
             (dict(Cd=129), UNSUPPORTED), (dict(E_=33, tau=tau), UNSUPPORTED), (dict(T=1 << 15, B=1 << 10), UNSUPPORTED)]
    table += [(dict(tau=t), INVALID) for t in bad_taus]
    table += [(dict(E_=33, tau=(C.c_float * 33)(*([0.0] * 33))), UNSUPPORTED)]       # the shape limits come before the values of tau are read
    for kw, want in table:
        assert votes(**kw) == want, sorted(kw)

    # bmi_ensemble_moments(logits, T, E, B, C, tau, Q1, Q2, QH, stream) and its _weighted / _vector / _matrix forms
    def moments(form="", T=2, E_=2, B=2, Cd=CD, tau=None, a=fake, b=fake, W=fake, logits=fake, Q1=fake):
        cal = {"": (tau,), "_weighted": (tau, W), "_vector": (a, b, W), "_matrix": (a, b, W)}[form]
        return getattr(lib, "bmi_ensemble_moments" + form)(logits, T, E_, B, Cd, *cal, Q1, fake, fake, None)

    for form in ("", "_weighted", "_vector", "_matrix"):
        table = [(dict(logits=None), INVALID), (dict(Q1=None), INVALID), (dict(T=0), INVALID), (dict(E_=33), UNSUPPORTED), (dict(Cd=129), UNSUPPORTED)]
        if form in ("_vector", "_matrix"):
            table += [(dict(a=None), INVALID), (dict(b=None), INVALID), (dict(W=None, E_=33), UNSUPPORTED)]
        else:
            table += [(dict(tau=(C.c_float * 2)(1.0, v)), INVALID) for v in (0.0, -1.0, float("nan"), float("inf"), 1e-45)]
        if form == "_weighted":
            table += [(dict(W=None), INVALID)]
        for kw, want in table:
            assert moments(form, **kw) == want, (form, sorted(kw))

    # bmi_engine_set_temperature / _vector_scaling / _matrix_scaling: arguments, then the exclusion in all six orders
    t4 = (C.c_float * 4)(0.5, 1.0, 2.0, 4.0)
    setters = {"temperature": (lambda: lib.bmi_engine_set_temperature(g.handle, t4, 4), lambda: lib.bmi_engine_set_temperature(g.handle, None, 0)),
               "vector": (lambda: lib.bmi_engine_set_vector_scaling(g.handle, fake, fake, E, CD), lambda: lib.bmi_engine_set_vector_scaling(g.handle, None, None, 0, 0)),
               "matrix": (lambda: lib.bmi_engine_set_matrix_scaling(g.handle, fake, fake, E, CD), lambda: lib.bmi_engine_set_matrix_scaling(g.handle, None, None, 0, 0))}
    assert lib.bmi_engine_set_temperature(None, ones, 4) == INVALID and lib.bmi_engine_set_temperature(g.handle, t4, 3) == INVALID
    for t in bad_taus:
        assert lib.bmi_engine_set_temperature(g.handle, t, 4) == INVALID
    for fn in (lib.bmi_engine_set_vector_scaling, lib.bmi_engine_set_matrix_scaling):
        assert fn(None, fake, fake, E, CD) == INVALID and fn(g.handle, fake, None, E, CD) == INVALID
        for e_, c_ in ((3, 10), (5, 10), (4, 9), (4, 100), (0, 0)):
            assert fn(g.handle, fake, fake, e_, c_) == INVALID
    for first, second in itertools.permutations(KINDS, 2):
        (set1, clear1), (set2, clear2) = setters[first], setters[second]
        assert set1() == OK
        assert set2() == INVALID, (first, second)
        assert clear2() == OK and set2() == INVALID                          # clearing what is not set is allowed and admits nothing
        if first != "temperature":
            assert lib.bmi_engine_set_temperature(g.handle, ones, 4) == OK   # all ones is no temperature: taken beside a scaling
        assert clear1() == OK
        assert set2() == OK and clear2() == OK                               # after clearing, the other kind sets
    assert lib.bmi_engine_set_temperature(g.handle, t4, 4) == OK and lib.bmi_engine_set_temperature(g.handle, ones, 4) == OK
    assert setters["vector"][0]() == OK and setters["vector"][1]() == OK     # all ones replaced the temperature: it is off
