"""-m gpu: the one key select behind the mass edges (csrc/record_common.h: radix_select_u32, launched as reliability.hip's line_edges_kernel)
serves both tables.  The same key buffer goes through the C ABI to bmi_reliability_table as keys [R][N + 3] and to bmi_classwise_table as
pkeys [R][1][N + 3] (C = 1, every label 0); by mass the two ``edges`` outputs and the np.sort-based edges of train.reliability agree bit
for bit.  Few distinct keys, so that duplicates straddle every digit pass of the select; N below n_bins (per = 0: every rank is 0) and one
chunk boundary of the table (N = 4097) are among the shapes."""
import ctypes as C

import numpy as np
import pytest
import torch

from bayesnn_fpga_amd import _lib
from bayesnn_fpga_amd.train.reliability import _mass_edges
from tests.gpu_helpers import ptr, stream

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
R, SPARE = 2, 3
# float32 bit patterns in (0, 1]: 0.25, 0.5, then keys that share 0.5's top 24, 16 and 8 bits, one that differs from it in two digits, and 1.0
VALUES = np.array([0x3E800000, 0x3F000000, 0x3F000001, 0x3F000100, 0x3F010000, 0x3F000101, 0x3F800000], dtype=np.uint32)


def make_keys(N, seed, equal=False):
    """uint32 [R][N + SPARE]: columns 0 .. N-1 drawn from VALUES (or all one value), the spare columns a key above every one of them"""
    rng = np.random.default_rng(seed)
    keys = np.full((R, N + SPARE), 0x3F800001, dtype=np.uint32)
    keys[:, :N] = VALUES[1] if equal else VALUES[rng.integers(0, len(VALUES), (R, N))]
    return keys


def both_tables(keys, N, n_bins, edges_in=None):
    """bmi_reliability_table and bmi_classwise_table over the same device buffer -> (edges [R][n_bins + 1] of each)"""
    lib, cap = _lib.lib(), keys.shape[1]
    k = torch.from_numpy(keys.view(np.int32)).to(DEV)
    hit = torch.zeros(R, cap, dtype=torch.uint8, device=DEV)
    f64 = torch.zeros(2, R, cap, dtype=torch.float64, device=DEV)
    labels = torch.zeros(cap, dtype=torch.int32, device=DEV)
    edges = torch.full((2, R, n_bins + 1), float("nan"), dtype=torch.float32, device=DEV)
    ints = torch.empty(2, 3, R, n_bins, dtype=torch.int64, device=DEV)
    sums = torch.empty(R, 2, dtype=torch.float64, device=DEV)
    valid = torch.empty(R, dtype=torch.int64, device=DEV)
    scratch = torch.empty(max(1, int(lib.bmi_reliability_scratch_bytes(R, N, n_bins))), dtype=torch.uint8, device=DEV)
    fixed = None if edges_in is None else (C.c_float * (n_bins + 1))(*[float(v) for v in edges_in])
    rc = lib.bmi_reliability_table(ptr(k), ptr(hit), ptr(f64[0]), ptr(f64[1]), R, N, cap, n_bins, fixed, ptr(edges[0]), ptr(ints[0, 0]),
                                   ptr(ints[0, 1]), ptr(ints[0, 2]), ptr(sums), ptr(scratch), scratch.numel(), stream())
    assert rc == _lib.BMI_OK
    rc = lib.bmi_classwise_table(ptr(k), ptr(labels), R, 1, N, cap, n_bins, fixed, ptr(edges[1]), ptr(ints[1, 0]), ptr(ints[1, 1]),
                                 ptr(ints[1, 2]), ptr(valid), stream())
    assert rc == _lib.BMI_OK
    torch.cuda.synchronize()
    got = edges.cpu().numpy()
    return got[0], got[1]


def assert_mass_edges(keys, N, n_bins):
    top, cw = both_tables(keys, N, n_bins)
    want = np.stack([_mass_edges(keys[r, :N], n_bins) for r in range(R)])
    assert np.array_equal(top.view(np.uint32), want.view(np.uint32))
    assert np.array_equal(cw.view(np.uint32), want.view(np.uint32))


@pytest.mark.parametrize("n_bins", [1, 2, 15, 64])
@pytest.mark.parametrize("N", [1, 2, 63, 257, 4097])
def test_mass_edges_of_both_tables_are_the_sorted_order_statistics(N, n_bins):
    assert_mass_edges(make_keys(N, 1000 * N + n_bins), N, n_bins)


def test_all_keys_equal():
    assert_mass_edges(make_keys(257, 0, equal=True), 257, 15)


def test_fixed_edges_are_the_callers():
    fixed = np.array([0.0, 0.25, 0.25, 0.5000001, 0.75, 1.0], dtype=np.float32)
    top, cw = both_tables(make_keys(63, 7), 63, 5, fixed)
    for got in (top, cw):
        assert np.array_equal(got.view(np.uint32), np.tile(fixed, (R, 1)).view(np.uint32))
