"""Uncertainty decomposition, CPU side: the reference's aPE pinned on its own fixtures, the float64 decomposition on the golden per-pass
logits, and the sharded collation of the packed S / H buffer under gloo with a CPU stand-in engine."""
import os
import socket

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

from bayesnn_fpga_amd.train.uncertainty import average_predictive_entropy, decompose_logits, entropy_rows
from tests.helpers import load_golden

GOLDEN_LOGITS = ["resnet18_exit_only", "resnet18_block_exit", "resnet18_layer_exit", "resnet18_mask4_block_exit", "resnet18_mask8_exit_c100",
                 "vgg19_exit_mc"]


def test_average_predictive_entropy_is_the_references():
    g = load_golden("uncertainty_ape.npz")
    names = [k[2:] for k in g.files if k.startswith("p_")]
    assert {"metrics", "peaky", "c100_exit0"} <= set(names)
    assert (g["p_peaky"] == 0).any()
    for n in names:
        assert abs(average_predictive_entropy(g[f"p_{n}"]) - float(g[f"ape_{n}"])) <= 1e-12, n


@pytest.mark.parametrize("name", GOLDEN_LOGITS)
def test_decomposition_bounds_on_golden_logits(name):
    logits = load_golden(f"{name}.npz")["logits"]                 # [T, E, B, C] fp32 per pass, from the reference
    C = logits.shape[-1]
    d = decompose_logits(logits)
    p = np.exp(logits.astype(np.float64) - logits.max(-1, keepdims=True))
    p /= p.sum(-1, keepdims=True)
    np.testing.assert_allclose(d["mean"], p.mean(0), rtol=0, atol=1e-15)
    np.testing.assert_allclose(d["exp_entropy"], entropy_rows(p).mean(0), rtol=0, atol=1e-12)
    mi, pe, ee = d["mutual_info"], d["pred_entropy"], d["exp_entropy"]
    assert (mi >= 0).all() and (mi <= pe + 1e-15).all() and (pe <= np.log(C) + 1e-12).all()
    assert (ee >= -1e-15).all() and (ee <= np.log(C) + 1e-12).all()
    # Jensen: the unclamped difference is itself non-negative (to rounding)
    assert (pe - ee >= -1e-12).all()


def test_decomposition_without_stochasticity_has_no_mutual_information():
    z = np.random.default_rng(0).standard_normal((3, 5, 10)) * 4
    d = decompose_logits(np.broadcast_to(z, (6,) + z.shape))
    assert np.abs(d["mutual_info"]).max() <= 1e-12
    np.testing.assert_allclose(d["pred_entropy"], d["exp_entropy"], rtol=0, atol=1e-12)
    peaky = decompose_logits(np.array([[[1e4, 0.0, -1e4]], [[0.0, 1e4, -1e4]]]))       # underflowed probabilities: no NaN
    assert np.isfinite(peaky["mutual_info"]).all() and abs(peaky["mutual_info"][0] - np.log(2)) < 1e-12


# ---- two gloo ranks, packed buffer, one all-reduce per batch -------------------------------------------------------------------
KW_MC = dict(dropout_exit=True, dropout="block", dropout_p=0.25, out_dim=10)


def _build():
    from bayesnn_fpga_amd.synthetic import synthetic_weights_
    from oracle.resnet18 import ResNet18MCEarlyExit
    torch.manual_seed(0)
    np.random.seed(0)
    return synthetic_weights_(ResNet18MCEarlyExit(**KW_MC), 0)


class _OracleEngine:
    """Stands in for MCDEngine (tests/test_sharding.py's stand-in, with the entropy sums H): the CPU oracle on the WHOLE batch, of which
    it returns the rows the call asked for."""
    n_exits, out_dim = 4, 10

    def __init__(self, model, x_full, seed):
        self.model, self.x_full, self.seed = model, x_full, seed

    def image_offset_ok(self, image_offset):
        return True

    def new_uncertainty_sums(self, batch):
        from bayesnn_fpga_amd.sharding import new_uncertainty_sums
        return new_uncertainty_sums(self.n_exits, batch, self.out_dim)

    def accumulate_uncertainty(self, x, S, H, t_begin, t_count, seed=0, cnt0=0, image_offset=0):
        from oracle import mcd
        assert torch.equal(x, self.x_full[image_offset:image_offset + x.shape[0]]) and seed == self.seed
        logits, probs = mcd.mcd_passes(self.model, self.x_full, t_count, seed, t_begin=t_begin)
        rows = slice(image_offset, image_offset + x.shape[0])
        S[0] += torch.from_numpy(probs.sum(0)[:, rows])
        S[1] += torch.from_numpy((probs ** 2).sum(0)[:, rows])
        S[2] += torch.from_numpy(logits.sum(0)[:, rows])
        H += torch.from_numpy(entropy_rows(probs).sum(0)[:, rows])
        return S, H


def _worker(rank, world, port, T, out_path):
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    import torch.distributed as dist
    dist.init_process_group("gloo", rank=rank, world_size=world)
    torch.set_num_threads(2)
    calls = []
    real = dist.all_reduce

    def counting(t, *a, **k):
        calls.append(t.numel())
        return real(t, *a, **k)
    dist.all_reduce = counting
    from bayesnn_fpga_amd.sharding import accumulate_partitioned_uncertainty, new_uncertainty_sums
    from bayesnn_fpga_amd.synthetic import synthetic_images
    x = synthetic_images(3, seed=1234)
    S, H = new_uncertainty_sums(4, 3, 10)
    accumulate_partitioned_uncertainty(_OracleEngine(_build(), x, 42), x, S, H, T, seed=42)
    dist.all_reduce = real
    if rank == 0:
        np.savez(out_path, S=S.numpy(), H=H.numpy(), calls=np.array(calls))
    dist.barrier()
    dist.destroy_process_group()


@pytest.mark.parametrize("T", [5, 1], ids=["samples", "images"])
def test_two_rank_gloo_packed_sums_equal_single_rank(tmp_path, T):
    """T = 5: the sample partition (ranks get 3 and 2 samples); T = 1 < world: the image partition (images [0, 2) and [2, 3))."""
    from bayesnn_fpga_amd.sharding import accumulate_partitioned_uncertainty, new_uncertainty_sums, partition
    from bayesnn_fpga_amd.synthetic import synthetic_images
    assert partition(T, 3, 0, 2)[0] == ("samples" if T == 5 else "images")
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    out = str(tmp_path / "SH.npz")
    mp.spawn(_worker, args=(2, port, T, out), nprocs=2, join=True)
    r = np.load(out)
    assert list(r["calls"]) == [3 * 4 * 3 * 10 + 4 * 3]          # ONE all-reduce, of the packed S + H buffer
    x = synthetic_images(3, seed=1234)
    S1, H1 = new_uncertainty_sums(4, 3, 10)
    accumulate_partitioned_uncertainty(_OracleEngine(_build(), x, 42), x, S1, H1, T, seed=42)     # no process group: one rank
    np.testing.assert_allclose(r["S"], S1.numpy(), rtol=1e-12, atol=1e-12)
    np.testing.assert_allclose(r["H"], H1.numpy(), rtol=1e-12, atol=1e-12)
    assert (r["H"] > 0).all()


def test_packed_views_are_checked():
    from bayesnn_fpga_amd.sharding import accumulate_partitioned_uncertainty
    with pytest.raises(ValueError, match="one buffer"):
        accumulate_partitioned_uncertainty(None, torch.zeros(1, 3, 32, 32), torch.zeros(3, 4, 1, 10, dtype=torch.float64),
                                           torch.zeros(4, 1, dtype=torch.float64), 2)


def test_library_binds_the_uncertainty_entry_points():
    from bayesnn_fpga_amd import _lib
    lib = _lib.lib()
    assert hasattr(lib, "bmi_forward_mcd_entropy") and hasattr(lib, "bmi_finalize_uncertainty")
    assert lib.bmi_forward_mcd_entropy(None, None, 1, 0, 0, 1, 0, 0, None, None, None, None, None, 0, None) == -22
    assert lib.bmi_finalize_uncertainty(1, 1, 10, 0, None, None, None, None, None, None, None) == -22
