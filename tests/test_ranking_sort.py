"""-m gpu: the sorted rank call (bmi_rank_quality_sorted, MCDEngine.rank_quality(method=)) against ``rank_quality_numpy`` and the detection
read-out (MCDEngine.rank_detection) against ``rank_detection_numpy``, bit for bit: around the sort's tile size, under keys that make every
one of the four digits decide, pure ties, invalid images and empty classes, and one row longer than the counting call takes."""
import numpy as np
import pytest
import torch

from bayesnn_fpga_amd import _lib
from bayesnn_fpga_amd.models.resnet18.resnet18 import ResNet18MCEarlyExit
from bayesnn_fpga_amd.synthetic import synthetic_weights_
from bayesnn_fpga_amd.train.ranking import INVALID, rank_detection_numpy, rank_quality_numpy
from tests.gpu_helpers import ptr, stream
from tests.helpers import build_seeded

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TILE = _lib.RANK_SORT_TILE
SPARE = 37                    # columns beyond N: never written
POISON = -7
OUTPUTS = ("rank", "sorted_keys", "curve", "counts", "aurc_sum")
LEVELS = np.array([0x00000001, 0x00000100, 0x00010000, 0x7F000000], dtype=np.uint32)
TPR = (0.5, 0.95, 1.0)


def inputs(R, N, keys, positives, seed=0):
    """ukeys uint32 [R, N + SPARE] and positive uint8 [R, N + SPARE]; the spare columns hold keys and bits that must not be read"""
    rng = np.random.default_rng(seed)
    shape = (R, N + SPARE)
    if keys == "equal":
        u = np.full(shape, 0x3F000000, dtype=np.uint32)
    elif keys == "digits":          # sums of a random subset of the four levels: 16 values, every digit decides some order
        u = (rng.integers(0, 2, shape + (4,)).astype(np.uint32) * LEVELS).sum(axis=-1, dtype=np.uint32)
    else:
        u = rng.integers(0, 1 << 31, shape, dtype=np.int64).astype(np.uint32)
        if keys == "invalid":       # a third of the columns invalid, in both spellings, and (R > 1) one row with no valid image
            u[:, 0::6], u[:, 3::6] = INVALID, 0x80000000
            u[R - 1 if R > 1 else R:] = INVALID
    u[:, N:] = 5
    p = {"random": rng.integers(0, 2, shape), "none": np.zeros(shape), "all": np.ones(shape)}[positives].astype(np.uint8)
    p[:, N:] = 1
    return u, p


def sorted_call(u, p, N):
    """bmi_rank_quality_sorted on poisoned outputs -> (the outputs' columns 0 .. N-1 as rank_quality_numpy shapes them, spare columns intact)"""
    R, cap = u.shape
    ud, pd = torch.from_numpy(u.view(np.int32)).to(DEV), torch.from_numpy(p).to(DEV)
    wide = torch.full((3, R, cap), POISON, dtype=torch.int32, device=DEV)
    counts = torch.full((R, 3), POISON, dtype=torch.int64, device=DEV)
    aurc = torch.full((R,), float("nan"), dtype=torch.float64, device=DEV)
    scratch = torch.empty(_lib.lib().bmi_rank_sort_scratch_bytes(R, N), dtype=torch.uint8, device=DEV)
    rc = _lib.lib().bmi_rank_quality_sorted(ptr(ud), ptr(pd), R, N, cap, ptr(wide[0]), ptr(wide[1]), ptr(wide[2]), ptr(counts), ptr(aurc),
                                            ptr(scratch), scratch.numel(), stream())
    torch.cuda.synchronize()
    assert rc == _lib.BMI_OK
    w = wide.cpu().numpy()
    got = dict(rank=w[0, :, :N], sorted_keys=np.ascontiguousarray(w[1, :, :N]).view(np.uint32), curve=w[2, :, :N], counts=counts.cpu().numpy(),
               aurc_sum=aurc.cpu().numpy())
    return got, bool((w[:, :, N:] == POISON).all())


def assert_same(got, want):
    for k in OUTPUTS:
        assert got[k].dtype == want[k].dtype and np.array_equal(got[k], want[k]), k
    assert got["aurc_sum"].tobytes() == want["aurc_sum"].tobytes()


@pytest.mark.parametrize("positives", ["random", "none", "all"])
@pytest.mark.parametrize("keys", ["equal", "digits", "random", "invalid"])
@pytest.mark.parametrize("R", [1, 3])
@pytest.mark.parametrize("N", [1, 255, TILE, TILE + 1, 3 * TILE + 17])
def test_sorted_call_equals_the_numpy_restatement(N, R, keys, positives):
    u, p = inputs(R, N, keys, positives, seed=N + R)
    got, intact = sorted_call(u, p, N)
    assert_same(got, rank_quality_numpy(u, p, N))
    assert intact
    if N == 3 * TILE + 17 and R == 3:                        # the same bits on every run
        again, _ = sorted_call(u, p, N)
        assert all(got[k].tobytes() == again[k].tobytes() for k in OUTPUTS)


@pytest.fixture(scope="module")
def engine():
    model = synthetic_weights_(build_seeded(ResNet18MCEarlyExit, dict(dropout_exit=True, dropout="block", dropout_p=0.25, out_dim=10)), 0)
    return model.to(DEV).eval().engine(torch.device(DEV), max_batch=8, dtype="f16x2")


def engine_table(engine, u, p, N, method):
    out = engine.rank_quality(torch.from_numpy(u.view(np.int32)).to(DEV), torch.from_numpy(p).to(DEV), N, method=method)
    torch.cuda.synchronize()
    got = {k: out[k].cpu().numpy()[..., :N] if k in OUTPUTS[:3] else out[k].cpu().numpy() for k in OUTPUTS}
    got["sorted_keys"] = np.ascontiguousarray(got["sorted_keys"]).view(np.uint32)
    return out, got


def test_auto_takes_a_row_longer_than_the_counting_call(engine):
    N = (1 << 17) + 4099
    rng = np.random.default_rng(5)
    u = np.zeros((1, N + SPARE), dtype=np.uint32)
    u[0, :N] = rng.integers(0, 1 << 31, N) % 1000
    p = rng.integers(0, 2, (1, N + SPARE)).astype(np.uint8)
    _, got = engine_table(engine, u, p, N, "auto")
    assert_same(got, rank_quality_numpy(u, p, N))
    with pytest.raises(ValueError):
        engine.rank_quality(torch.from_numpy(u.view(np.int32)).to(DEV), torch.from_numpy(p).to(DEV), N, method="count")


@pytest.mark.parametrize("N,R,keys,positives", [(255, 3, "digits", "random"), (255, 3, "invalid", "random"), (TILE + 1, 1, "digits", "none"),
                                                (TILE + 1, 1, "equal", "all")])
def test_detection_equals_the_numpy_restatement(engine, N, R, keys, positives):
    u, p = inputs(R, N, keys, positives, seed=11)
    table, got = engine_table(engine, u, p, N, "sort")
    want = rank_detection_numpy(dict(got, n=N), TPR)
    det = engine.rank_detection(table, TPR)
    assert det["tpr"] == TPR and np.array_equal(det["det"].cpu().numpy(), want["det"])
    assert det["ap_sum"].cpu().numpy().tobytes() == want["ap_sum"].tobytes()
