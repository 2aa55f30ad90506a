"""-m gpu: the one rule of the calibration maps on an engine, as a table over the kinds (temperature, vector, matrix) — ResNet-18 multi-exit,
out_dim 10, B = 3, T = 2, E = 4.  While one kind is in force every other setter raises and leaves the engine's results untouched; after
clearing, the other kind sets; ensemble_moments and vote_counts with the map passed as arguments equal the engine-set results exactly; a
BatchesInFlight setter of each kind leaves no captured graph."""
import itertools

import numpy as np
import pytest
import torch

from bayesnn_fpga_amd.engine import BatchesInFlight, MCDEngine
from bayesnn_fpga_amd.models.resnet18.resnet18 import ResNet18MCEarlyExit
from bayesnn_fpga_amd.synthetic import synthetic_images, synthetic_weights_
from tests.helpers import build_seeded

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
KW = dict(dropout_exit=True, dropout="block", dropout_p=0.25, out_dim=10)
B, T, E, CD, SEED = 3, 2, 4, 10, 11
_rng = np.random.default_rng(5)
# kind -> (the engine's setter, its arguments, the same map as the keyword arguments of ensemble_moments / vote_counts)
MAPS = {"temperature": ("set_temperature", ([0.5, 1.25, 2.0, 4.0],), dict(tau=[0.5, 1.25, 2.0, 4.0]))}
_a, _b = _rng.uniform(0.4, 2.2, (E, CD)), _rng.uniform(-1, 1, (E, CD))
MAPS["vector"] = ("set_vector_scaling", (_a, _b), dict(scale=_a, bias=_b))
_m = np.eye(CD) * _a[:, :, None] + _rng.uniform(-0.1, 0.1, (E, CD, CD))
MAPS["matrix"] = ("set_matrix_scaling", (_m, _b), dict(matrix=_m, bias=_b))
KINDS = tuple(MAPS)


@pytest.fixture(scope="module")
def model():
    return synthetic_weights_(build_seeded(ResNet18MCEarlyExit, KW), 0).to(DEV).eval()


@pytest.fixture(scope="module")
def x():
    return synthetic_images(B, seed=12).to(DEV)


@pytest.fixture()
def eng(model):
    e = MCDEngine(model, DEV, max_batch=B, dtype="f16")
    yield e
    e.close()


def _same(r0, r1):
    return set(r0) == set(r1) and all(torch.equal(r0[k], r1[k]) for k in r0)


def _votes(eng, x):
    r = eng.predict_votes(x, T, seed=SEED)
    torch.cuda.synchronize()
    return {k: v.clone() for k, v in r.items()}


@pytest.mark.parametrize("first,second", list(itertools.permutations(KINDS, 2)))
def test_a_map_in_force_refuses_the_other_setters_and_keeps_its_results(eng, x, first, second):
    plain = _votes(eng, x)
    set1, args1, _ = MAPS[first]
    set2, args2, _ = MAPS[second]
    getattr(eng, set1)(*args1)
    before = _votes(eng, x)
    assert not torch.equal(before["mean"], plain["mean"]) and torch.equal(before["logit_mean"], plain["logit_mean"])
    with pytest.raises(ValueError):
        getattr(eng, set2)(*args2)
    assert _same(before, _votes(eng, x))                                    # the refused call left the engine as it was
    getattr(eng, set2)(None)                                                # clearing what is not set is allowed and changes nothing
    assert _same(before, _votes(eng, x))
    getattr(eng, set1)(None)
    assert _same(plain, _votes(eng, x))                                     # off: the bits of an engine that never had a map
    getattr(eng, set2)(*args2)                                              # after clearing, the other kind sets
    assert not torch.equal(_votes(eng, x)["mean"], plain["mean"])
    assert (eng.vector_scaling is not None) == (second == "vector") and (eng.matrix_scaling is not None) == (second == "matrix")
    assert (eng.temperature != [1.0] * E) == (second == "temperature")


@pytest.mark.parametrize("weighted", [False, True], ids=["mean", "weighted"])
@pytest.mark.parametrize("kind", KINDS)
def test_held_logits_with_the_map_as_arguments_equal_the_engine_set_results(eng, x, kind, weighted):
    w = [1.0, 2.0, 3.0, 4.0] if weighted else None
    logits = eng.forward_samples(x, T, seed=SEED)
    setter, args, given = MAPS[kind]
    getattr(eng, setter)(*args)
    eng.set_ensemble_weights(w)
    r = _votes(eng, x)
    getattr(eng, setter)(None)                                              # the arguments are independent of what is set on the engine
    eng.set_ensemble_weights(None)
    m = eng.ensemble_moments(logits, weights=w, **given)
    V = eng.vote_counts(logits, weights=w, **given)
    torch.cuda.synchronize()
    for k in ("ens_mean", "ens_var", "ens_pred_entropy", "ens_exp_entropy", "ens_mutual_info"):
        assert torch.equal(m[k], r[k]), k
    assert torch.equal(V[0], r["votes"]) and torch.equal(V[1], r["ens_votes"])
    with pytest.raises(ValueError):
        eng.vote_counts(logits, **{**MAPS[KINDS[(KINDS.index(kind) + 1) % 3]][2], **given})      # two maps at once
    with pytest.raises(ValueError):
        eng.ensemble_moments(logits, bias=_b)


@pytest.mark.parametrize("kind", KINDS)
def test_a_pipe_setter_leaves_no_captured_graph(model, x, kind):
    pipe = BatchesInFlight(model, DEV, n=1, max_batch=B, dtype="f16")
    try:
        r0 = pipe.predict_graphed(x, T, SEED)
        pipe.synchronize()
        r0 = {k: v.clone() for k, v in r0.items()}
        assert hasattr(pipe, "_graphs")
        setter, args, _ = MAPS[kind]
        getattr(pipe, setter)(*args)
        assert not hasattr(pipe, "_graphs") and not hasattr(pipe, "_gstreams")
        r1 = pipe.predict_graphed(x, T, SEED)
        pipe.synchronize()
        eager = pipe.engines[0].predict(x, T, seed=SEED)
        torch.cuda.synchronize()
        assert all(torch.equal(r1[k], eager[k]) for k in eager) and not torch.equal(r1["mean"], r0["mean"])
    finally:
        pipe.close()
