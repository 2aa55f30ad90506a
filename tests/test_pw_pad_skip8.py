"""-m gpu: the pad-skip form of conv3x3_pw on 8x8 maps ("pw_pad_skip8" = 1: a workgroup tile of the persistent kernel is 16 images x one
4x4 quadrant of the map, an MFMA pixel tile one output position across the 16 images, so a (position, tap) pair that reads the
zero-padding ring is a whole tile that is never read or multiplied and the ring is never fetched) against the 4 x 4-block form
("pw_pad_skip8" = 0).  A product with an all-zero pixel fragment leaves its accumulator as it was and the K order is the same, so every
output must be bitwise equal: the plain epilogue, the fused 1x1 shortcut, the BasicBlock tails (no site / 2-bit elementwise site /
Masksembles), fp16 and bf16, on the S3 shape (256 -> 256 on 8x8) with N = 3 and 5 (fewer images than one tile), 16 (exactly one group
of 16), 37 (ragged last group, fewer tiles than CUs) and 4101 (several tiles per CU, ragged last group); through the engine, the
headline model's moments and the dynamic-exit entry."""
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
CIN, COUT, H = 256, 256, 8          # S3: layer3's stride-1 convs
NS = [3, 5, 16, 37, 4101]


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
    """Process defaults for the single-kernel entry points: conv3x3_pw without its minimum-grid rule (the persistent walk), the element type."""
    def __init__(self, dt):
        self.dt = dt

    def __enter__(self):
        _lib.set_option("conv_pw", 2)
        if self.dt == "bf16":
            _lib.set_option("unit_entry_dtype", _lib.DTYPE_BF16)

    def __exit__(self, *exc):
        _lib.set_option("pw_pad_skip8", 1)
        _lib.set_option("conv_pw", 1)
        _lib.set_option("unit_entry_dtype", _lib.DTYPE_F16)


def _same_bits(outs):
    a, b = (o.view(torch.int16) for o in outs)
    assert torch.isfinite(outs[0].float()).all() and float(outs[0].float().abs().max()) > 0
    assert torch.equal(a, b), f"{int((a != b).sum())} of {a.numel()} elements differ"


@pytest.mark.parametrize("dt", ["f16", "bf16"])
@pytest.mark.parametrize("shortcut", [False, True])
@pytest.mark.parametrize("n", NS)
def test_plain_epilogue_and_fused_shortcut(n, shortcut, dt):
    lib = _lib.lib()
    tdt = torch.bfloat16 if dt == "bf16" else torch.float16
    g, x, w, scale, bias = _operands(n, tdt, 17)
    x2 = torch.randn(n, 2 * H, 2 * H, CIN // 2, generator=g).to(tdt).to(DEV) if shortcut else None
    w2 = (torch.randn(COUT, CIN // 2, generator=g) * (2.0 / CIN) ** 0.5).to(tdt).to(DEV) if shortcut else None
    outs = []
    with _unit_options(dt):
        for skip in (0, 1):
            _lib.set_option("pw_pad_skip8", skip)
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


@pytest.mark.parametrize("dt", ["f16", "bf16"])
@pytest.mark.parametrize("use_site", [0, 1, 2])
@pytest.mark.parametrize("n", NS)
def test_residual_tails(n, use_site, dt):
    """BN + residual + ReLU, alone (0), with the 2-bit elementwise site (1: the Philox keep bits are indexed by image and position) and with
    Masksembles (2); batch = 7 makes the sample index change inside a tile."""
    tdt = torch.bfloat16 if dt == "bf16" else torch.float16
    g, x, w, scale, bias = _operands(n, tdt, 23)
    res = torch.randn(n, H, H, COUT, generator=g).to(tdt).to(DEV)
    site = dict(kind=_lib.SITE_ELEMENTWISE, site_id=2, p=0.25) if use_site == 1 else None
    if use_site == 2:
        site = dict(kind=_lib.SITE_MASKSEMBLE, site_id=1, masks=(torch.rand(4, COUT, generator=g) < 0.6).float().numpy() * 1.5)
    outs = []
    with _unit_options(dt):
        for skip in (0, 1):
            _lib.set_option("pw_pad_skip8", skip)
            outs.append(gh.run_conv(x, w, scale, bias, res, True, 1, 1, n, n, n, site=site, batch=7, t0=3, seed=9, cnt0=2, out_dtype=tdt))
    _same_bits(outs)
    if use_site:
        assert float((outs[0] == 0).float().mean()) > 0.25            # dropped elements (and ReLU zeros)
    if use_site == 0 and dt == "f16" and n <= 37:
        ref = gh.conv_ref(x, w, scale, bias, res, True, 1, 1, n, n, n)
        torch.testing.assert_close(outs[1].float().cpu().permute(0, 3, 1, 2), ref, rtol=2e-3, atol=3e-3)


def _engine(B, T, dt, mask_type):
    m = build_seeded(ResNet18MCEarlyExit, dict(dropout_exit=True, dropout="block", dropout_p=0.25, out_dim=10, mask_type=mask_type))
    synthetic_weights_(m, 0)
    eng = m.to(DEV).eval().engine(torch.device(DEV), max_batch=B, chunk_samples=T, dtype=dt)
    eng.set_option("conv_pw", 2)          # conv3x3_pw whatever the grid: the small batches too
    return eng


@pytest.mark.parametrize("mask_type", ["mc", "mask"])
@pytest.mark.parametrize("dt", ["f16", "bf16"])
@pytest.mark.parametrize("B,T", [(5, 1), (16, 2), (37, 3), (250, 4)])
def test_headline_model_through_the_engine(B, T, dt, mask_type):
    """layer3 of the headline model (MC dropout: the 2-bit site in conv2's tail; Masksembles: the mask table) with B x T = 5, 32, 111 (ragged
    last group of 16) and 1000 images per launch: the same moments in every exit."""
    eng = _engine(B, T, dt, mask_type)
    x = synthetic_images(B, seed=1234).to(DEV)
    outs = []
    for skip in (0, 1):
        eng.set_option("pw_pad_skip8", skip)
        outs.append(eng.predict(x, T, seed=5))
    for k in ("mean", "var", "logit_mean"):
        assert torch.isfinite(outs[0][k]).all()
        assert torch.equal(outs[0][k], outs[1][k]), k


@pytest.mark.parametrize("dt", ["f16", "bf16"])
def test_dynamic_exit_entry(dt):
    """After the first tested exit the launches carry a row table and stay on the 4 x 4-block tiles in both settings; the launches before it
    take the quadrant tiles: same exits, same bits for the images that go on."""
    B, T = 45, 6
    eng = _engine(B, T, dt, "mc")
    x = synthetic_images(B, seed=21).to(DEV)
    conf = eng.predict(x, T, seed=11)["mean"].max(-1).values
    for thr in (float(conf[1].median()), float(conf[2].quantile(0.3)), 1.0):
        outs = []
        for skip in (0, 1):
            eng.set_option("pw_pad_skip8", skip)
            outs.append(eng.predict_with_exit(x, T, thr, seed=11))
        assert outs[0]["active_after"] == outs[1]["active_after"]
        assert torch.equal(outs[0]["exit_layer"], outs[1]["exit_layer"])
        assert torch.equal(outs[0]["best_preds"], outs[1]["best_preds"])
        got = outs[0]["exit_layer"].cpu().numpy()
        for e in range(1, 4):                 # rows of exits an image never reached are meaningless
            keep = torch.from_numpy(np.nonzero(got >= e)[0]).to(DEV)
            for k in ("mean", "var"):
                assert torch.equal(outs[0][k][e][keep], outs[1][k][e][keep]), (thr, e, k)
