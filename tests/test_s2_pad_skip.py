"""-m gpu: the pad-skip form of conv3x3_s2 on 8x8 -> 4x4 maps ("s2_pad_skip" = 1: an MFMA pixel tile is one output position across the
tile's 16 images and the cells of a parity plane are stored position-major, so a (position, tap) pair that reads only the padding row or
column is a whole tile that is never read or multiplied) against the 4 x 4-block form ("s2_pad_skip" = 0).  A product with an all-zero
pixel fragment leaves its accumulator as it was and the K order is the same, so every output must be bitwise equal: the single conv
(64 -> 256: two chunks, the chunk hand-over; 256 -> 512) and the pair (128 -> 256+256, 256 -> 512+512), fp16 and bf16, with N = 3 and 5
(fewer images than a tile), 16 (one tile), 37 (ragged) and 4101 (several tiles per workgroup, ragged last); through the engine, the
headline model's moments with the pooled epilogue (launches that pool, and the pair of which one conv pools) and with "conv_pool" = 0,
and the dynamic-exit entry (row-table launches stay on the 4 x 4-block form)."""
import numpy as np
import pytest
import torch

from bayesnn_fpga_amd import _lib
from bayesnn_fpga_amd.models.resnet18.resnet18 import ResNet18MCEarlyExit
from bayesnn_fpga_amd.synthetic import synthetic_images, synthetic_weights_
from tests import gpu_helpers as gh
from tests.helpers import build_seeded

pytestmark = [pytest.mark.gpu, pytest.mark.usefixtures("fp16_engine_default")]
DEV = "cuda:0"
H = 8
NS = [3, 5, 16, 37, 4101]


def _gen(seed):
    g = torch.Generator()
    g.manual_seed(seed)
    return g


def _conv_operands(g, cin, cout, tdt):
    w = (torch.randn(cout, 3, 3, cin, generator=g) * (2.0 / (9 * cin)) ** 0.5).to(tdt).to(DEV)
    return w, (0.5 + torch.rand(cout, generator=g)).to(DEV), (0.2 * torch.randn(cout, generator=g)).to(DEV)


class _unit_options:
    """Process defaults for the single-kernel entry points: conv3x3_s2 without its minimum-grid rule, the element type."""
    def __init__(self, dt):
        self.dt = dt

    def __enter__(self):
        _lib.set_option("conv_s2", 2)
        if self.dt == "bf16":
            _lib.set_option("unit_entry_dtype", _lib.DTYPE_BF16)

    def __exit__(self, *exc):
        _lib.set_option("s2_pad_skip", 1)
        _lib.set_option("conv_s2", 1)
        _lib.set_option("unit_entry_dtype", _lib.DTYPE_F16)


def _same_bits(a, b):
    assert torch.isfinite(a.float()).all() and float(a.float().abs().max()) > 0
    ai, bi = a.view(torch.int16), b.view(torch.int16)
    assert torch.equal(ai, bi), f"{int((ai != bi).sum())} of {ai.numel()} elements differ"


@pytest.mark.parametrize("dt", ["f16", "bf16"])
@pytest.mark.parametrize("cin,cout", [(64, 256), (256, 512)])
@pytest.mark.parametrize("n", NS)
def test_single_conv(n, cin, cout, dt):
    lib = _lib.lib()
    tdt = torch.bfloat16 if dt == "bf16" else torch.float16
    g = _gen(31)
    x = torch.randn(n, H, H, cin, generator=g).to(tdt).to(DEV)
    w, scale, bias = _conv_operands(g, cin, cout, tdt)
    outs = []
    with _unit_options(dt):
        for skip in (0, 1):
            _lib.set_option("s2_pad_skip", skip)
            out = torch.full((n, H // 2, H // 2, cout), float("nan"), dtype=tdt, device=DEV)
            _lib.check(lib.bmi_conv_igemm_fwd(gh.ptr(x), None, 1.0, gh.ptr(w), gh.ptr(scale), gh.ptr(bias), None, gh.ptr(out), n, n, n, H, H, cin, cout, 3, 2, 1, 1,
                                              None, n, 0, 0, 0, gh.stream()), "bmi_conv_igemm_fwd")
            torch.cuda.synchronize()
            outs.append(out)
    _same_bits(*outs)
    if dt == "f16" and n <= 37:      # ... and both are the convolution
        ref = gh.conv_ref(x, w, scale, bias, None, True, 2, 1, n, n, n)
        torch.testing.assert_close(outs[1].float().cpu().permute(0, 3, 1, 2), ref, rtol=2e-3, atol=3e-3)


@pytest.mark.parametrize("dt", ["f16", "bf16"])
@pytest.mark.parametrize("cin,cout", [(128, 256), (256, 512)])
@pytest.mark.parametrize("n", NS)
def test_pair(n, cin, cout, dt):
    """Two convs of cout channels each on one input, one launch."""
    lib = _lib.lib()
    tdt = torch.bfloat16 if dt == "bf16" else torch.float16
    g = _gen(37)
    x = torch.randn(n, H, H, cin, generator=g).to(tdt).to(DEV)
    ops = [_conv_operands(g, cin, cout, tdt) for _ in range(2)]
    runs = []
    with _unit_options(dt):
        for skip in (0, 1):
            _lib.set_option("s2_pad_skip", skip)
            outs = [torch.full((n, H // 2, H // 2, cout), float("nan"), dtype=tdt, device=DEV) for _ in range(2)]
            _lib.check(lib.bmi_conv_pair_fwd(gh.ptr(x), gh.ptr(ops[0][0]), gh.ptr(ops[0][1]), gh.ptr(ops[0][2]), gh.ptr(outs[0]), gh.ptr(ops[1][0]), gh.ptr(ops[1][1]),
                                             gh.ptr(ops[1][2]), gh.ptr(outs[1]), n, n, H, H, cin, cout, cout, 3, 2, 1, 1, gh.stream()), "bmi_conv_pair_fwd")
            torch.cuda.synchronize()
            runs.append(outs)
    for i in range(2):
        _same_bits(runs[0][i], runs[1][i])


def _engine(B, T, dt, mask_type):
    m = build_seeded(ResNet18MCEarlyExit, dict(dropout_exit=True, dropout="block", dropout_p=0.25, out_dim=10, mask_type=mask_type))
    synthetic_weights_(m, 0)
    eng = m.to(DEV).eval().engine(torch.device(DEV), max_batch=B, chunk_samples=T, dtype=dt)
    eng.set_option("conv_s2", 2)          # conv3x3_s2 whatever the grid: the small batches too
    return eng


@pytest.mark.parametrize("conv_pool", [1, 0])
@pytest.mark.parametrize("mask_type", ["mc", "mask"])
@pytest.mark.parametrize("dt", ["f16", "bf16"])
@pytest.mark.parametrize("B,T", [(5, 1), (16, 2), (37, 3), (250, 4)])
def test_headline_model_through_the_engine(B, T, dt, mask_type, conv_pool):
    """The exit-head convs of the headline model pool their 4x4 map in the epilogue (the pad-skip form sums an image's 16 positions across
    the two pixel waves through LDS), layer4's pair stores one conv plainly and pools the other; conv_pool = 0: every one stores its map."""
    eng = _engine(B, T, dt, mask_type)
    eng.set_option("conv_pool", conv_pool)
    x = synthetic_images(B, seed=1234).to(DEV)
    outs = []
    for skip in (0, 1):
        eng.set_option("s2_pad_skip", skip)
        outs.append(eng.predict(x, T, seed=5))
    for k in ("mean", "var", "logit_mean"):
        assert torch.isfinite(outs[0][k]).all()
        assert k == "var" or float(outs[0][k].abs().max()) > 0          # (the variance of T = 1 sample is zero)
        assert torch.equal(outs[0][k], outs[1][k]), k


@pytest.mark.parametrize("dt", ["f16", "bf16"])
def test_dynamic_exit_entry(dt):
    """After the first tested exit the launches carry a row table and stay on the 4 x 4-block tiles in both settings; the launches before it
    take the pad-skip form: same exits, same bits for the images that go on."""
    B, T = 45, 6
    eng = _engine(B, T, dt, "mc")
    x = synthetic_images(B, seed=21).to(DEV)
    conf = eng.predict(x, T, seed=11)["mean"].max(-1).values
    for thr in (float(conf[1].median()), float(conf[2].quantile(0.3)), 1.0):
        outs = []
        for skip in (0, 1):
            eng.set_option("s2_pad_skip", skip)
            outs.append(eng.predict_with_exit(x, T, thr, seed=11))
        assert outs[0]["active_after"] == outs[1]["active_after"]
        assert torch.equal(outs[0]["exit_layer"], outs[1]["exit_layer"])
        assert torch.equal(outs[0]["best_preds"], outs[1]["best_preds"])
        got = outs[0]["exit_layer"].cpu().numpy()
        for e in range(1, 4):                 # rows of exits an image never reached are meaningless
            keep = torch.from_numpy(np.nonzero(got >= e)[0]).to(DEV)
            for k in ("mean", "var"):
                assert torch.equal(outs[0][k][e][keep], outs[1][k][e][keep]), (thr, e, k)
