"""-m gpu: the pad-skip form of conv3x3_pw on 4x4 maps ("pw_pad_skip" = 1: an MFMA pixel tile is one output position across the 16
images of a workgroup tile, so a (position, tap) pair that reads the zero-padding ring is a whole tile that is never fetched, read or
multiplied) against the 4 x 4-block form ("pw_pad_skip" = 0).  A product with an all-zero pixel fragment leaves its accumulator as it
was and the K order is the same, so every output must be bitwise equal: the plain epilogue, the fused 1x1 shortcut, the BasicBlock
tails (no site / 2-bit elementwise site / Masksembles), the pooled tail and the dynamic-exit row-table form, fp16 and bf16, on the
S4 shape (512 -> 512 on 4x4) with N = 5 (fewer images than one tile), 16 (exactly one), 37 (ragged last tile, fewer tiles than CUs)
and 4101 (several tiles per CU, ragged last tile) — in the persistent and in the per-tile kernel."""
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
CIN, COUT, H = 512, 512, 4          # S4: layer4's stride-1 convs
NS = [5, 16, 37, 4101]


def _gen(seed):
    g = torch.Generator()
    g.manual_seed(seed)
    return g


def _operands(n, tdt, seed):
    g = _gen(seed)
    x = torch.randn(n, H, H, CIN, generator=g).to(tdt).to(DEV)
    w = (torch.randn(COUT, 3, 3, CIN, generator=g) * (2.0 / (9 * CIN)) ** 0.5).to(tdt).to(DEV)
    scale, bias = (0.5 + torch.rand(COUT, generator=g)).to(DEV), (0.2 * torch.randn(COUT, generator=g)).to(DEV)
    return g, x, w, scale, bias


class _unit_options:
    """Process defaults for the single-kernel entry points: conv3x3_pw without its minimum-grid rule, the element type, the walk."""
    def __init__(self, dt, persist):
        self.dt, self.persist = dt, persist

    def __enter__(self):
        _lib.set_option("conv_pw", 2)
        _lib.set_option("pw_persist", self.persist)
        if self.dt == "bf16":
            _lib.set_option("unit_entry_dtype", _lib.DTYPE_BF16)

    def __exit__(self, *exc):
        _lib.set_option("pw_pad_skip", 1)
        _lib.set_option("pw_persist", 1)
        _lib.set_option("conv_pw", 1)
        _lib.set_option("unit_entry_dtype", _lib.DTYPE_F16)


def _same_bits(outs):
    a, b = (o.view(torch.int16) for o in outs)
    assert torch.isfinite(outs[0].float()).all() and float(outs[0].float().abs().max()) > 0
    assert torch.equal(a, b), f"{int((a != b).sum())} of {a.numel()} elements differ"


@pytest.mark.parametrize("persist", [1, 0])
@pytest.mark.parametrize("dt", ["f16", "bf16"])
@pytest.mark.parametrize("shortcut", [False, True])
@pytest.mark.parametrize("n", NS)
def test_plain_epilogue_and_fused_shortcut(n, shortcut, dt, persist):
    lib = _lib.lib()
    tdt = torch.bfloat16 if dt == "bf16" else torch.float16
    g, x, w, scale, bias = _operands(n, tdt, 17)
    x2 = torch.randn(n, 2 * H, 2 * H, CIN // 2, generator=g).to(tdt).to(DEV) if shortcut else None
    w2 = (torch.randn(COUT, CIN // 2, generator=g) * (2.0 / CIN) ** 0.5).to(tdt).to(DEV) if shortcut else None
    outs = []
    with _unit_options(dt, persist):
        for skip in (0, 1):
            _lib.set_option("pw_pad_skip", skip)
            out = torch.full((n, H, H, COUT), float("nan"), dtype=tdt, device=DEV)
            if shortcut:
                _lib.check(lib.bmi_conv3x3_shortcut_fwd(gh.ptr(x), gh.ptr(w), gh.ptr(x2), gh.ptr(w2), gh.ptr(bias), gh.ptr(out), n, H, H, CIN, COUT, CIN // 2, 1,
                                                        gh.stream()), "bmi_conv3x3_shortcut_fwd")
            else:
                _lib.check(lib.bmi_conv_igemm_fwd(gh.ptr(x), None, 1.0, gh.ptr(w), gh.ptr(scale), gh.ptr(bias), None, gh.ptr(out), n, n, n, H, H, CIN, COUT, 3, 1, 1, 1,
                                                  None, n, 0, 0, 0, gh.stream()), "bmi_conv_igemm_fwd")
            torch.cuda.synchronize()
            outs.append(out)
    _same_bits(outs)
    if not shortcut and dt == "f16" and n <= 37:      # ... and both are the convolution
        ref = gh.conv_ref(x, w, scale, bias, None, True, 1, 1, n, n, n)
        torch.testing.assert_close(outs[1].float().cpu().permute(0, 3, 1, 2), ref, rtol=2e-3, atol=3e-3)


@pytest.mark.parametrize("persist", [1, 0])
@pytest.mark.parametrize("dt", ["f16", "bf16"])
@pytest.mark.parametrize("use_site", [0, 1, 2])
@pytest.mark.parametrize("n", NS)
def test_residual_tails(n, use_site, dt, persist):
    """BN + residual + ReLU, alone (0), with the 2-bit elementwise site (1: the Philox keep bits are indexed by image and position) and with
    Masksembles (2); batch = 7 makes the sample index change inside a tile."""
    tdt = torch.bfloat16 if dt == "bf16" else torch.float16
    g, x, w, scale, bias = _operands(n, tdt, 23)
    res = torch.randn(n, H, H, COUT, generator=g).to(tdt).to(DEV)
    site = dict(kind=_lib.SITE_ELEMENTWISE, site_id=2, p=0.25) if use_site == 1 else None
    if use_site == 2:
        site = dict(kind=_lib.SITE_MASKSEMBLE, site_id=1, masks=(torch.rand(4, COUT, generator=g) < 0.6).float().numpy() * 1.5)
    outs = []
    with _unit_options(dt, persist):
        for skip in (0, 1):
            _lib.set_option("pw_pad_skip", skip)
            outs.append(gh.run_conv(x, w, scale, bias, res, True, 1, 1, n, n, n, site=site, batch=7, t0=3, seed=9, cnt0=2, out_dtype=tdt))
    _same_bits(outs)
    if use_site:
        assert float((outs[0] == 0).float().mean()) > 0.25            # dropped elements (and ReLU zeros)


def _engine(B, T, dt):
    m = build_seeded(ResNet18MCEarlyExit, dict(dropout_exit=True, dropout="block", dropout_p=0.25, out_dim=10))
    synthetic_weights_(m, 0)
    eng = m.to(DEV).eval().engine(torch.device(DEV), max_batch=B, chunk_samples=T, dtype=dt)
    eng.set_option("conv_pw", 2)          # conv3x3_pw whatever the grid: the small batches too
    return eng


@pytest.mark.parametrize("dt", ["f16", "bf16"])
@pytest.mark.parametrize("B,T", [(5, 1), (16, 1), (37, 1), (1367, 3)])
def test_pooled_tail_through_the_engine(B, T, dt):
    """layer4[1].conv2 feeds nothing but the final head: its tail writes fp32 means over the 4x4 map ("conv_pool").  In the pad-skip form an
    image's 16 positions are registers of two waves, summed through LDS in the order of the 4 x 4-block form's DPP tree: the same bits in
    every moment of every exit (the launch carries B x T images: 5, 16, 37, 4101)."""
    eng = _engine(B, T, dt)
    x = synthetic_images(B, seed=1234).to(DEV)
    outs = []
    for skip in (0, 1):
        eng.set_option("pw_pad_skip", skip)
        outs.append(eng.predict(x, T, seed=5))
    for k in ("mean", "var", "logit_mean"):
        assert torch.isfinite(outs[0][k]).all()
        assert torch.equal(outs[0][k], outs[1][k]), k
    eng.set_option("conv_pool", 0)        # the pooled tail did run: without the fusion the final exit rounds its map to 16 bits
    assert not torch.equal(eng.predict(x, T, seed=5)["mean"][3], outs[1]["mean"][3])


@pytest.mark.parametrize("dt", ["f16", "bf16"])
@pytest.mark.parametrize("B,T", [(45, 6), (250, 4)])
def test_dynamic_exit_row_table_form(B, T, dt):
    """After the first tested exit the launches carry a row table (compact image index -> tensor row / Philox image index) and run the per-tile
    kernel's IMAP instantiations on however many images are still active: same exits, same bits."""
    eng = _engine(B, T, dt)
    x = synthetic_images(B, seed=21).to(DEV)
    conf = eng.predict(x, T, seed=11)["mean"].max(-1).values
    for thr in (float(conf[1].median()), float(conf[2].quantile(0.3)), 1.0):
        outs = []
        for skip in (0, 1):
            eng.set_option("pw_pad_skip", skip)
            outs.append(eng.predict_with_exit(x, T, thr, seed=11))
        assert outs[0]["active_after"] == outs[1]["active_after"]
        assert torch.equal(outs[0]["exit_layer"], outs[1]["exit_layer"])
        assert torch.equal(outs[0]["best_preds"], outs[1]["best_preds"])
        got = outs[0]["exit_layer"].cpu().numpy()
        for e in range(1, 4):                 # rows of exits an image never reached are meaningless
            keep = torch.from_numpy(np.nonzero(got >= e)[0]).to(DEV)
            for k in ("mean", "var"):
                assert torch.equal(outs[0][k][e][keep], outs[1][k][e][keep]), (thr, e, k)
    assert outs[0]["active_after"][2] == B    # threshold 1.0: every image went through every stage with a row table
