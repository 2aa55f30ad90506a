"""Every conv kernel against an integer reference, bit for bit: non-square, odd and tiny maps, k in {1, 3, 5}, strides 1-3, pads 0-2,
ragged and large launches, every engine dtype (tests/exact_ops.py builds operands whose arithmetic is exact, so no tolerance is needed
and n = 4101 is checked element by element like n = 3).  Inputs and outputs sit between NaN flanks: a write outside a tensor, an element
left unwritten or a consumed read from outside an input fails the case.

Each case states its outcome, taken from the launchers: "ok" (BMI_OK, equal to the reference, flanks intact) or a decline
(BMI_ERR_UNSUPPORTED and an untouched output).  A decline is expected only where no kernel of the dtype takes the channel counts: the
16-bit kernels need Cin % 64 == 0 and Cout % 64 == 0 (conv_igemm, the last in launch_conv's chain), conv_split and conv_exact
Cin % 32 == 0 and Cout % 64 == 0; a shape one of the specialised kernels declines must come out exact through the kernel behind it.

The CPU part (no gpu marker) checks the operands themselves: every committed case passes the reference's own assertions (abs(acc) < 2^24,
representable in the output type), fp32 torch agrees with float64, the operands can see an indexing error, the guard sees a write."""
import ctypes as C
from dataclasses import replace

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from bayesnn_fpga_amd import _lib
from oracle import philox
from tests import exact_ops as xo
from tests import gpu_helpers as gh
from tests.exact_ops import Case

gpu = pytest.mark.gpu
B16 = ("f16", "bf16")
ELEM5, ELEM0, ELEM75, ELEM1, CHAN5, CHAN75, MSK = ("elem", 0.5), ("elem", 0.0), ("elem", 0.75), ("elem", 1.0), ("chan", 0.5), ("chan", 0.75), ("msk",)

# both MFMA shapes of conv3x3_patch / conv_igemm_wide, the 16x16x32 one with the lite and with the general epilogue
MFMA = {"mfma32": dict(mfma_shape_patch=32, mfma_shape_wide=32), "mfma16": dict(mfma_shape_patch=16, mfma_shape_wide=16),
        "mfma16-general": dict(mfma_shape_patch=16, mfma_shape_wide=16, epilogue_lite=0)}


def declined_for(c, dtype):
    """The one table of expected declines of bmi_conv_igemm_fwd (see the module docstring)."""
    if dtype in B16:
        return c.cin % 64 != 0 or c.cout % 64 != 0
    return c.cin % 32 != 0 or c.cout % 64 != 0


# ---- (a) general geometry: conv_igemm, conv_igemm_wide, conv_split, conv_exact -------------------------------------------------------
# M = n * Ho * Wo below one 128-pixel tile, exactly one, and ragged over several; in_mod / res_mod < n; every epilogue term on and off
GENERAL = [
    Case(64, 64, 5, 7, n=3, res=True, site=ELEM5, batch=2),                                       # M = 105: below one tile
    Case(64, 128, 7, 5, stride=2, n=9, in_mod=3, res=True, res_mod=3),                            # stride 2 on an odd map: 4x3 (floor)
    Case(128, 64, 1, 1, k=1, pad=0, n=128, scale=False, bias=False, relu=False),                  # M = 128: exactly one tile
    Case(128, 256, 2, 2, n=37, site=CHAN75, batch=5),                                             # M = 148
    Case(64, 128, 1, 9, n=29, site=MSK, batch=5, res=True),                                       # one row: M = 261
    Case(64, 64, 1, 9, k=1, stride=3, pad=0, n=50, bias=False),                                   # 1x3 outputs
    Case(128, 128, 3, 32, n=4, res=True, site=ELEM0, batch=3),                                    # M = 384: three whole tiles
    Case(64, 256, 3, 32, k=5, stride=2, pad=2, n=5, relu=False),                                  # 2x16 outputs
    Case(128, 64, 12, 20, k=5, pad=2, n=3, res=True, site=ELEM75, batch=2),                       # M = 720
    Case(64, 128, 12, 20, stride=3, pad=0, n=11, scale=False),                                    # 4x6 outputs, M = 264
    Case(128, 256, 12, 20, k=1, stride=2, pad=0, n=7, in_mod=2, site=CHAN5, batch=2),             # 6x10 outputs
    Case(64, 128, 33, 31, n=2, res=True, res_mod=1, site=ELEM1, batch=1),                         # M = 2046; p = 1 drops everything
    Case(128, 256, 33, 31, stride=2, n=3, res=True, site=MSK, batch=2),                           # 17x16 outputs
    Case(64, 64, 33, 31, k=5, stride=3, pad=2, n=2),                                              # 11x11 outputs
    Case(64, 64, 33, 31, pad=0, n=1, res=True),                                                   # pad != (k - 1) / 2: 31x29
    Case(64, 128, 5, 7, k=1, pad=1, n=3, res=True),                                               # 1x1 with padding: a bias-only border, 7x9
    Case(64, 64, 5, 7, pad=2, n=5, site=ELEM5, batch=3),                                          # 3x3 with pad 2: 7x9
    Case(128, 128, 5, 7, k=5, pad=0, n=44),                                                       # 1x3 outputs, M = 132
    Case(64, 256, 2, 2, stride=2, n=300, res=True, site=ELEM5, batch=7),                          # 1x1 outputs, M = 300
    Case(128, 64, 1, 1, k=5, pad=2, n=300, in_mod=7),                                             # only the centre tap is inside the map
    Case(64, 128, 7, 5, k=5, stride=2, pad=1, n=6),                                               # 2x1 outputs
    Case(128, 256, 33, 31, n=49),                                                                 # 196 x 256-pixel tiles: conv_igemm_wide (persistent form), ragged
    Case(128, 256, 12, 20, n=205, res=True, site=ELEM5, batch=9),                                 # ... its lite / general epilogues, M = 49200
    Case(64, 256, 12, 20, k=5, stride=2, pad=2, n=821, site=MSK, batch=10),                       # ... 6x10 outputs, M = 49260
    Case(64, 128, 33, 31, n=101),                                                                 # conv_igemm's 256-pixel tiles (>= 400 of them)
    Case(32, 64, 5, 7, n=3),                                                                      # Cin % 64: declined by the 16-bit kernels only
    Case(96, 128, 7, 5, k=1, pad=0, n=20, res=True),                                              # ... (96 = 3 x 32)
    Case(64, 32, 5, 7, n=3),                                                                      # Cout % 64: declined everywhere
]


def _general_params():
    out = []
    for c in GENERAL:
        for dt in xo.DTYPES:
            if dt not in B16:
                out.append(pytest.param(c, dt, {}, id=f"{c.id}-{dt}"))
                continue
            for name, o in MFMA.items():
                for wide in ((1, 0) if c.cout % 256 == 0 else (1,)):     # (conv_igemm_wide takes Cout % 256 == 0 only)
                    out.append(pytest.param(c, dt, dict(o, conv_wide=wide), id=f"{c.id}-{dt}-{name}" + ("" if wide else "-nowide")))
    return out


# ---- (b) conv3x3_patch's row bands: Ho % 8 == 0 and Wo == 32 -------------------------------------------------------------------------
def _patch_cases():
    out = []
    for H in (8, 16, 24, 32):
        out += [Case(64, 128, H, 32, n=3), Case(128, 128, H, 32, n=2, res=True, site=ELEM5, batch=1),
                Case(64, 128, H, 32, n=3, in_mod=1, res=True, res_mod=2, site=MSK, batch=2), Case(128, 128, H, 32, n=2, scale=False, bias=False, relu=False),
                Case(64, 64, H, 32, n=3, res=True, site=ELEM75, batch=2), Case(64, 64, H, 32, n=2, site=CHAN5, batch=1)]
    # declined neighbours: exact through conv_igemm
    for H, W in ((8, 16), (12, 32), (32, 16)):
        out += [Case(64, 128, H, W, n=3, res=True, site=ELEM5, batch=2), Case(64, 64, H, W, n=3)]
    return out


def _patch_params():
    out = []
    for c in _patch_cases():
        for dt in B16:
            for name, o in MFMA.items():
                for p64 in ((1, 0) if c.cout == 64 else (1,)):
                    out.append(pytest.param(c, dt, dict(o, conv_patch64=p64), id=f"{c.id}-{dt}-{name}" + ("" if p64 else "-nopatch64")))
    return out


# ---- (c) the specialised kernels at their own shapes, at size ------------------------------------------------------------------------
PW_OPTS = {"persist-skip": dict(pw_persist=1, pw_pad_skip=1, pw_pad_skip8=1), "tile-blocks": dict(pw_persist=0, pw_pad_skip=0, pw_pad_skip8=0),
           "persist-blocks": dict(pw_persist=1, pw_pad_skip=0, pw_pad_skip8=0), "tile-skip": dict(pw_persist=0, pw_pad_skip=1, pw_pad_skip8=1)}
SIZES = (1, 3, 16, 37)


def _sized(make, big, opt_sets, big_opt_sets, fixed):
    """make(n) for the small sizes under every option set and for the large ragged `big` under `big_opt_sets`, f16 and bf16."""
    out = []
    for n in SIZES + (big,):
        c = make(n)
        for name in (opt_sets if n != big else big_opt_sets):
            for dt in B16:
                out.append(pytest.param(c, dt, dict(fixed, **opt_sets[name]), id=f"{c.id}-{dt}-{name}"))
    return out


def _pw_params():
    out, fx = [], dict(conv_pw=2)
    both = ("persist-skip", "tile-blocks")
    out += _sized(lambda n: Case(128, 256, 8, 8, n=n), 1031, PW_OPTS, both, fx)
    out += _sized(lambda n: Case(64, 256, 8, 8, n=n, res=True, site=ELEM5, batch=min(n, 7)), 2111, PW_OPTS, both, fx)
    out += _sized(lambda n: Case(128, 256, 4, 4, n=n), 4101, PW_OPTS, both, fx)
    out += _sized(lambda n: Case(64, 512, 4, 4, n=n, res=True, site=MSK, batch=min(n, 7)), 4101, PW_OPTS, both, fx)
    out += _sized(lambda n: Case(128, 256, 4, 4, n=n, in_mod=max(1, n // 3), res=True, res_mod=max(1, n // 2), site=CHAN5, batch=min(n, 5)), 1031, PW_OPTS, both, fx)
    # declined neighbours (ho != wo): exact through the kernels behind conv3x3_pw
    for H, W in ((8, 4), (4, 8)):
        for n in (3, 37, 1031):
            for c in (Case(128, 256, H, W, n=n), Case(64, 256, H, W, n=n, res=True, site=ELEM5, batch=min(n, 7))):
                out += [pytest.param(c, dt, dict(fx), id=f"{c.id}-{dt}") for dt in B16]
    return out


def _s2_params():
    out, fx, one = [], dict(conv_s2=2), {"s2": {}}
    out += _sized(lambda n: Case(64, 128, 32, 32, stride=2, n=n), 1031, one, one, fx)                       # the 128-channel tiles of the 16x16 outputs
    out += _sized(lambda n: Case(64, 256, 32, 32, stride=2, n=n, in_mod=max(1, n // 2)), 1031, one, one, fx)  # input broadcast (16x16 outputs only)
    out += _sized(lambda n: Case(64, 256, 16, 16, stride=2, n=n), 2111, one, one, fx)
    out += _sized(lambda n: Case(128, 512, 8, 8, stride=2, n=n, bias=False), 4101, one, one, fx)
    out += _sized(lambda n: Case(64, 128, 32, 32, stride=2, n=n, entry="pair", cout_b=128), 1031, one, one, fx)
    out += _sized(lambda n: Case(64, 128, 16, 16, stride=2, n=n, entry="pair", cout_b=128), 2111, one, one, fx)
    out += _sized(lambda n: Case(128, 256, 8, 8, stride=2, n=n, entry="pair", cout_b=256), 4101, one, one, fx)
    # declined neighbours: 16x8 outputs (ho != wo) and odd inputs (h != 2 * ho): exact through conv_igemm_wide / conv_igemm
    for H, W in ((32, 16), (31, 31), (15, 16)):
        for n in (3, 37, 1031):
            c = Case(64, 256, H, W, stride=2, n=n)
            out += [pytest.param(c, dt, dict(fx), id=f"{c.id}-{dt}") for dt in B16]
    c = Case(64, 128, 32, 16, stride=2, n=37, entry="pair", cout_b=128)
    out += [pytest.param(c, dt, dict(fx), id=f"{c.id}-{dt}") for dt in B16]
    return out


def _stream_params():
    out, fx, one = [], dict(conv_stream=2), {"stream": {}}
    k1 = dict(k=1, pad=0)
    out += _sized(lambda n: Case(64, 128, 5, 7, n=n, **k1), 2111, one, one, fx)                                              # plain; odd, non-square
    out += _sized(lambda n: Case(128, 256, 33, 31, stride=2, n=n, **k1), 101, one, one, fx)                                  # stride 2 on an odd map: 17x16
    out += _sized(lambda n: Case(256, 128, 8, 8, n=n, res=True, **k1), 1031, one, one, fx)                                   # residual + ReLU on the registers
    out += _sized(lambda n: Case(64, 256, 7, 5, n=n, res=True, site=ELEM5, batch=min(n, 7), **k1), 2111, one, one, fx)       # ... + the 2-bit site
    out += _sized(lambda n: Case(128, 128, 3, 32, n=n, in_mod=max(1, n // 2), res=True, res_mod=max(1, n // 3), site=MSK, batch=min(n, 5), **k1), 1031, one, one, fx)
    out += _sized(lambda n: Case(512, 128, 2, 2, stride=2, n=n, site=CHAN75, batch=min(n, 5), **k1), 4101, one, one, fx)     # general epilogue: declined, conv_igemm
    return out


def _seam_params():
    out, fx, one = [], dict(conv_seam=2), {"seam": {}}
    k1 = dict(k=1, pad=0, res=True, entry="seam")
    out += _sized(lambda n: Case(64, 256, 5, 7, n=n, cn=128, **k1), 1031, one, one, fx)
    out += _sized(lambda n: Case(128, 512, 8, 8, n=n, cn=128, **k1), 1031, one, one, fx)
    out += _sized(lambda n: Case(64, 128, 4, 4, n=n, cn=256, relu=False, **k1), 4101, one, one, fx)
    c = Case(64, 256, 5, 7, n=37, cn=64, **k1)                # cn = 64: declined by the seam kernel, the two launches
    out += [pytest.param(c, dt, dict(fx), id=f"{c.id}-{dt}") for dt in B16]
    return out


def _shortcut_params():
    out = []
    sc = dict(entry="shortcut", scale=False)
    out += _sized(lambda n: Case(128, 256, 8, 8, n=n, cin2=64, **sc), 1031, PW_OPTS, ("persist-skip", "tile-blocks"), dict(conv_pw=2))
    out += _sized(lambda n: Case(128, 256, 4, 4, n=n, cin2=128, **sc), 4101, PW_OPTS, ("persist-skip", "tile-blocks"), dict(conv_pw=2))
    out += _sized(lambda n: Case(64, 128, 16, 16, n=n, cin2=64, **sc), 1031, MFMA, ("mfma16",), {})                 # conv3x3_patch
    out += _sized(lambda n: Case(128, 256, 8, 8, n=n, cin2=64, relu=False, **sc), 1031, MFMA, ("mfma16",), dict(conv_pw=0))
    out += _sized(lambda n: Case(64, 128, 8, 32, n=n, cin2=64, **sc), 101, MFMA, ("mfma16",), {})                   # ... a row band
    return out


# ---- CPU part: the operands ----------------------------------------------------------------------------------------------------------
def _all_committed():
    """(case, dtype) of every GPU parameter above, once."""
    seen, out = set(), []
    for p in _general_params() + _patch_params() + _pw_params() + _s2_params() + _stream_params() + _seam_params() + _shortcut_params():
        c, dt = p.values[0], p.values[1]
        if (c, dt) not in seen:
            seen.add((c, dt))
            out.append((c, dt))
    return sorted(out, key=lambda v: (v[0].id, xo.flavour_for(v[1])))       # (consecutive dtypes of a case share the cached float64 work)


def test_every_committed_case_is_exact_in_its_output_type():
    """exact_reference's own assertions — abs(acc) < 2^24, unchanged by a cast to the output type and back — for every case, seed and dtype
    the GPU part runs; and the outputs are not trivial (most of them nonzero unless a site drops everything)."""
    pairs = _all_committed()
    assert len(pairs) > 500
    for c, dt in pairs:
        refs = xo.exact_reference(c, dt)
        for r in refs:
            assert r.shape[0] == c.n and torch.isfinite(r).all()
            if c.site != ELEM1:
                assert float((r != 0).double().mean()) > 0.05, (c.id, dt)


SMALL = [c for c in GENERAL + _patch_cases()[:6] if c.n <= 50]


@pytest.mark.parametrize("flavour", ["dense", "bounded"])
def test_fp32_torch_conv_equals_float64(flavour):
    for c in SMALL:
        o = xo.exact_operands(c, flavour)
        x, w = o["x"].permute(0, 3, 1, 2), o["w"].permute(0, 3, 1, 2)
        y32 = F.conv2d(x.float(), w.float(), stride=c.stride, padding=c.pad)
        y64 = F.conv2d(x, w, stride=c.stride, padding=c.pad)
        assert torch.equal(y32.double(), y64), c.id
        assert torch.equal(xo.conv64(o["x"], o["w"], c.stride, c.pad), y64), c.id
        if flavour == "bounded":
            assert int((o["w"] != 0).reshape(c.cout, -1).sum(1).max()) <= xo.NNZ and float(y64.abs().max()) <= xo.NNZ
            if c.cout * xo.NNZ >= c.k * c.k * c.cin:              # every (ky, kx, cin) position is used by some channel
                assert bool((o["w"] != 0).any(0).all()), c.id


@pytest.mark.parametrize("flavour", ["dense", "bounded"])
def test_operands_see_an_indexing_error(flavour):
    """A reference with one input column shifted, or (dense weights, k > 1) one tap's weights moved to the neighbouring tap, differs from the
    true one in at least one element of EVERY output channel: a kernel with such an error cannot pass.  On maps of at least 2x2 whose
    outputs see more than one input column."""
    tried = 0
    for c in SMALL:
        if c.H < 2 or c.W < 2 or c.ho * c.wo * c.n < 8 or c.cin % 64:
            continue
        o = xo.exact_operands(c, flavour)
        y = xo.conv64(o["x"], o["w"], c.stride, c.pad)
        xs = o["x"].clone()
        col = min(c.W - 1, c.pad + 1) if c.stride == 1 else 0          # a column every geometry reads
        xs[:, :, col] = o["x"][:, :, (col + 1) % c.W]
        d = (xo.conv64(xs, o["w"], c.stride, c.pad) != y)
        assert bool(d.permute(1, 0, 2, 3).reshape(c.cout, -1).any(1).all()), f"{c.id}: column shift"
        tried += 1
        if flavour == "dense" and c.k > 1:
            ws = o["w"].clone()
            ky = kx = c.k // 2                                         # the centre tap is inside every map
            ws[:, ky, kx], ws[:, ky, kx - 1] = o["w"][:, ky, kx - 1] * 0, o["w"][:, ky, kx - 1] + o["w"][:, ky, kx]
            d = (xo.conv64(o["x"], ws, c.stride, c.pad) != y)
            assert bool(d.permute(1, 0, 2, 3).reshape(c.cout, -1).any(1).all()), f"{c.id}: moved tap"
    assert tried >= 15


def test_guard_detects_a_write_into_a_flank():
    t = torch.arange(2 * 3 * 5 * 8, dtype=torch.float32).reshape(2, 3, 5, 8)
    for where in ("before", "after", "far"):
        g = xo.guarded(t)
        assert g.flank >= 256 * 8 and g.flank >= 3 * 5 * 8 and g.flanks_intact() and torch.equal(g.body, t)
        assert g.body.data_ptr() == g.buf.data_ptr() + 4 * g.flank
        at = dict(before=g.flank - 1, after=g.flank + t.numel(), far=len(g.buf) - 1)[where]
        g.buf[at] = 0.0
        assert not g.flanks_intact()
    o = xo.guarded_like((2, 3, 5, 8), torch.float16, "cpu")
    assert bool(torch.isnan(o.body).all()) and o.flanks_intact()
    o.body[1, 2, 4, 7] = 1.0                        # a write inside the body is none of the guard's business
    assert o.flanks_intact()
    b = xo.guarded_like((64,), torch.uint8, "cpu", fill=0xA5)
    assert b.flanks_intact()
    b.buf[b.flank + 64] = 0
    assert not b.flanks_intact()


# ---- GPU part ------------------------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("case,dtype,opts", _general_params())
def test_general_geometry(case, dtype, opts):
    xo.check_exact(case, dtype, "declined" if declined_for(case, dtype) else "ok", opts)


@gpu
@pytest.mark.parametrize("case,dtype,opts", _patch_params())
def test_row_band_patch_kernel(case, dtype, opts):
    xo.check_exact(case, dtype, "ok", opts)


@gpu
@pytest.mark.parametrize("case,dtype,opts", _pw_params())
def test_conv3x3_pw_at_size(case, dtype, opts):
    xo.check_exact(case, dtype, "ok", opts)


@gpu
@pytest.mark.parametrize("case,dtype,opts", _s2_params())
def test_conv3x3_s2_and_pair_at_size(case, dtype, opts):
    xo.check_exact(case, dtype, "ok", opts)


@gpu
@pytest.mark.parametrize("case,dtype,opts", _stream_params())
def test_conv1x1_stream_at_size(case, dtype, opts):
    xo.check_exact(case, dtype, "ok", opts)


@gpu
@pytest.mark.parametrize("case,dtype,opts", _seam_params())
def test_conv1x1_seam_at_size(case, dtype, opts):
    xo.check_exact(case, dtype, "ok", opts)


@gpu
@pytest.mark.parametrize("case,dtype,opts", _shortcut_params())
def test_conv3x3_shortcut_at_size(case, dtype, opts):
    xo.check_exact(case, dtype, "ok", opts)


@gpu
@pytest.mark.parametrize("dtype", B16)
def test_shortcut_entry_declines_a_map_no_fused_kernel_takes(dtype):
    """The fused shortcut lives in conv3x3_pw and conv3x3_patch only (conv_igemm refuses ConvArgs::in2): a 5x7 map is declined, untouched."""
    xo.check_exact(Case(64, 128, 5, 7, n=3, cin2=64, entry="shortcut", scale=False), dtype, "declined")


@gpu
def test_pair_entry_declines_the_exact_engine():
    xo.check_exact(Case(64, 128, 16, 16, stride=2, n=3, entry="pair", cout_b=128), "f32", "declined")


# ---- (d) the non-conv ops on the same geometries -------------------------------------------------------------------------------------
def _int_tensor(rng, shape, lo=-4, hi=4):
    return torch.from_numpy(rng.integers(lo, hi + 1, size=shape).astype(np.float64))


@gpu
@pytest.mark.parametrize("dtype", xo.DTYPES)
@pytest.mark.parametrize("H,W,k,stride,pad,cout,n,expect", [(5, 7, 3, 1, 1, 64, 9, "ok"), (5, 7, 5, 2, 2, 32, 3, "ok"), (33, 31, 3, 2, 1, 64, 2, "ok"),
                                                            (33, 31, 5, 1, 0, 32, 1, "ok"), (33, 31, 5, 1, 2, 64, 1, "declined")])
def test_stem_conv_exact(dtype, H, W, k, stride, pad, cout, n, expect):
    """bmi_stem_conv_fwd: fp32 NCHW in, Cin = 3, every output dtype; 64 x 5 x 5 x 3 weights exceed its 4096-float LDS table: declined."""
    rng = np.random.default_rng(5)
    x = torch.from_numpy(rng.integers(-1, 2, size=(n, 3, H, W)).astype(np.float64))
    w = torch.from_numpy(rng.integers(-1, 2, size=(cout, k, k, 3)).astype(np.float64))
    scale, bias = torch.from_numpy(rng.choice([0.5, 1.0, 2.0], size=cout)), _int_tensor(rng, (cout,))
    ref = torch.relu(F.conv2d(x, w.permute(0, 3, 1, 2), stride=stride, padding=pad) * scale[None, :, None, None] + bias[None, :, None, None])
    assert torch.equal(xo.roundtrip(ref, dtype), ref) and (ref > 0).any()
    ho, wo = ref.shape[2:]
    xg, wg, sg, bg = xo.guarded(x.float(), gh.DEV), xo.guarded(w.float(), gh.DEV), xo.guarded(scale.float(), gh.DEV), xo.guarded(bias.float(), gh.DEV)
    out = xo._out(n, ho, wo, cout, dtype, gh.DEV)
    with xo.options(unit_entry_dtype=_lib.DTYPES[dtype]):
        rc = _lib.lib().bmi_stem_conv_fwd(gh.ptr(xg.body), gh.ptr(wg.body), gh.ptr(sg.body), gh.ptr(bg.body), gh.ptr(out.body), n, 3, H, W, cout, k, stride, pad, 1,
                                          gh.stream())
        torch.cuda.synchronize()
    assert all(g.flanks_intact() for g in (xg, wg, sg, bg, out))
    got = xo._decode(out, dtype)
    if expect == "declined":
        assert rc == xo.UNSUPPORTED and bool(torch.isnan(got).all())
    else:
        assert rc == _lib.BMI_OK and torch.equal(got, ref.permute(0, 2, 3, 1))


@gpu
@pytest.mark.parametrize("dtype", xo.DTYPES)
@pytest.mark.parametrize("H,W,c,n,expect", [(6, 10, 64, 5, "ok"), (2, 8, 96, 3, "ok"), (10, 2, 32, 37, "ok"), (5, 7, 64, 3, "declined"), (6, 7, 64, 3, "declined"),
                                            (7, 6, 64, 3, "declined")])
def test_maxpool2_geometry(dtype, H, W, c, n, expect):
    """bmi_maxpool2 takes even maps only, square or not (launch_maxpool2: (h & 1) || (w & 1) is declined).  The reference model's
    MaxPool2d(2) floors an odd map; no model of the path pools one, and the kernel refuses it instead of flooring: nothing is written."""
    rng = np.random.default_rng(6)
    x = _int_tensor(rng, (n, H, W, c), -100, 100)
    xg, out = xo._act(x, dtype, gh.DEV), xo._out(n, H // 2, W // 2, c, dtype, gh.DEV)
    with xo.options(unit_entry_dtype=_lib.DTYPES[dtype]):
        rc = _lib.lib().bmi_maxpool2(gh.ptr(xg.body), gh.ptr(out.body), n, H, W, c, gh.stream())
        torch.cuda.synchronize()
    assert xg.flanks_intact() and out.flanks_intact()
    got = xo._decode(out, dtype)
    if expect == "declined":
        assert rc == xo.UNSUPPORTED and bool(torch.isnan(got).all())
    else:
        assert rc == _lib.BMI_OK and torch.equal(got, F.max_pool2d(x.permute(0, 3, 1, 2), 2).permute(0, 2, 3, 1))


@gpu
@pytest.mark.parametrize("dtype", xo.DTYPES)
@pytest.mark.parametrize("p", [0.0, 0.5, 0.75, 1.0])
@pytest.mark.parametrize("hw,c,B,tc,in_stoch", [(35, 64, 3, 4, False), (1, 64, 5, 3, True), (35, 96, 2, 3, True), (1, 96, 7, 2, False)])
def test_mask_apply_exact(dtype, p, hw, c, B, tc, in_stoch):
    """bmi_mask_apply on hw = 35 (a 5x7 map) and hw = 1, C = 64 and 96 (every kernel takes C % 32 == 0): integers times a multiplier in
    {0, 1, 2, 4} — equal to the oracle's mask bit for bit, expanding (input [B]) and same-size launches."""
    rng = np.random.default_rng(7)
    n, n_in = B * tc, (B * tc if in_stoch else B)
    H, W = (5, 7) if hw == 35 else (1, 1)
    x = _int_tensor(rng, (n_in, H, W, c), -30, 30)
    site = dict(kind=_lib.SITE_ELEMENTWISE, site_id=3, p=p)
    keep = []
    s = gh.site_struct(site, keep)
    xg, out = xo._act(x, dtype, gh.DEV), xo._out(n, H, W, c, dtype, gh.DEV)
    with xo.options(unit_entry_dtype=_lib.DTYPES[dtype]):
        rc = _lib.lib().bmi_mask_apply(gh.ptr(xg.body), gh.ptr(out.body), n, n_in, hw, c, C.byref(s), B, xo.T0, xo.SEED, 0, gh.stream())
        torch.cuda.synchronize()
    assert rc == _lib.BMI_OK and xg.flanks_intact() and out.flanks_intact()
    mult = gh.folded_site_mask(site, B, c, H, W, tc, xo.T0, xo.SEED).double()
    ref = (x.permute(0, 3, 1, 2)[torch.arange(n) % n_in] * mult).permute(0, 2, 3, 1)
    assert torch.equal(xo.roundtrip(ref, dtype), ref)
    assert torch.equal(xo._decode(out, dtype), ref)
    assert bool((mult == 0).all()) == (p == 1.0) and bool((mult != 0).all()) == (p == 0.0)


@gpu
@pytest.mark.parametrize("p", [0.0, 0.5, 0.75, 1.0])
@pytest.mark.parametrize("hw,c,B,tc", [(35, 64, 3, 4), (1, 64, 5, 3), (35, 96, 2, 3), (1, 96, 8, 2)])
def test_mask_bits_exact(p, hw, c, B, tc):
    n = B * tc
    s = gh.site_struct(dict(kind=_lib.SITE_ELEMENTWISE, site_id=2, p=p), [])
    bits = xo.guarded_like((n * hw * c // 8,), torch.uint8, gh.DEV, fill=0xA5)
    rc = _lib.lib().bmi_mask_bits(gh.ptr(bits.body), n, hw, c, C.byref(s), B, xo.T0, xo.SEED, gh.stream())
    torch.cuda.synchronize()
    assert rc == _lib.BMI_OK and bits.flanks_intact()
    want = np.concatenate([philox.keep_bits(B * hw * c, xo.SEED, 2, xo.T0 + tl, p) for tl in range(tc)])
    assert np.array_equal(np.unpackbits(bits.body.cpu().numpy(), bitorder="little").astype(bool), want)


@gpu
@pytest.mark.parametrize("in_kind", ["f16", "bf16", "f32"])
@pytest.mark.parametrize("k,cout,n,in_mod,site", [(32, 64, 1, 1, None), (32, 64, 131, 131, ELEM5), (96, 192, 131, 7, ELEM75), (96, 64, 37, 37, MSK), (32, 192, 300, 3, None)])
def test_dense_f32_exact(in_kind, k, cout, n, in_mod, site):
    """bmi_dense_f32 on integers: K and Cout at their smallest (32, 64) and at a non-power-of-two multiple (96, 192); ragged n."""
    rng = np.random.default_rng(8)
    x, w, b = _int_tensor(rng, (in_mod, k), -1, 1), _int_tensor(rng, (cout, k), -1, 1), _int_tensor(rng, (cout,))
    B = 7 if n > 7 else n
    sd = xo.site_dict(Case(k, cout, 1, 1, site=site), cout)
    keep = []
    s = gh.site_struct(sd, keep)
    xg = xo.guarded(x.float() if in_kind == "f32" else x.to(xo.T16[in_kind]), gh.DEV)
    wg, bg = xo.guarded(w.float(), gh.DEV), xo.guarded(b.float(), gh.DEV)
    out = xo.guarded_like((n, cout), torch.float32, gh.DEV)
    with xo.options(unit_entry_dtype=_lib.DTYPES["bf16" if in_kind == "bf16" else "f16"]):
        rc = _lib.lib().bmi_dense_f32(gh.ptr(xg.body), int(in_kind == "f32"), gh.ptr(wg.body), gh.ptr(bg.body), gh.ptr(out.body), n, in_mod, k, cout, 1,
                                      C.byref(s) if s is not None else None, B, xo.T0, xo.SEED, xo.CNT0, gh.stream())
        torch.cuda.synchronize()
    assert rc == _lib.BMI_OK and all(g.flanks_intact() for g in (xg, wg, bg, out))
    ref = torch.relu(x[torch.arange(n) % in_mod] @ w.T + b)
    if sd is not None:
        ref = ref * gh.folded_site_mask(sd, B, cout, 1, 1, -(-n // B), xo.T0, xo.SEED, xo.CNT0)[:n].reshape(n, cout).double()
    assert torch.equal(out.body.double().cpu(), ref)
