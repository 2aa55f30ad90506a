"""Exact-arithmetic operands, float64 references and guarded allocations for the conv kernels (tests/test_conv_exact_geometry.py).

With activations and weights in {-1, 0, 1}, power-of-two BN scales, small integer bias / residual and site multipliers in {0, 1, 2, 4},
every product and every partial sum of a conv is an integer far below 2^24 in whatever order an MFMA adds them, the epilogue is exact in
fp32 and the result is representable in the output type: a kernel's output must equal the reference bit for bit, at any batch size.
A plain module like tests/gpu_helpers.py: no fixtures; options are set through the `options` context manager."""
import contextlib
import ctypes as C
import functools
from dataclasses import dataclass, replace

import numpy as np
import torch
import torch.nn.functional as F

from bayesnn_fpga_amd import _lib
from tests import gpu_helpers as gh

UNSUPPORTED = -95                       # BMI_ERR_UNSUPPORTED
DTYPES = ("f16", "bf16", "f32", "f16x2", "bf16x3")
T16 = {"f16": torch.float16, "bf16": torch.bfloat16, "f16x2": torch.float16, "bf16x3": torch.bfloat16}
POOL = 64                               # distinct images of a large batch (the others repeat them by index)
POOL_MACS = 3e9                         # ... fewer for the heavy geometries: what one reference conv may cost
NNZ = 24                                # nonzero weights per output channel of the bounded flavour
SEED, T0, CNT0 = (7 << 32) + 42, 3, 2   # Philox seed, first sample index, first Masksembles row of every launch

# the process defaults of the kernel-selection switches (csrc/kernels.h, BmiOptions) that `options` puts back
DEFAULTS = dict(unit_entry_dtype=_lib.DTYPE_F16, mfma_shape_patch=0, mfma_shape_wide=0, epilogue_lite=1, conv_wide=1, conv_pw=1, pw_persist=1,
                pw_pad_skip=1, pw_pad_skip8=1, conv_s2=1, conv_stream=1, conv_seam=1, conv_patch64=1)


@contextlib.contextmanager
def options(**kw):
    """bmi_set_option for the block; every switch goes back to its default whatever happens inside."""
    try:
        for k, v in kw.items():
            assert k in DEFAULTS, k
            _lib.set_option(k, v)
        yield
    finally:
        for k in kw:
            _lib.set_option(k, DEFAULTS[k])


@dataclass(frozen=True)
class Case:
    """One launch.  entry: "conv" (bmi_conv_igemm_fwd), "pair" (bmi_conv_pair_fwd: cout + cout_b channels), "shortcut"
    (bmi_conv3x3_shortcut_fwd: + a 1x1 stride-2 conv of cin2 channels on the 2H x 2W map), "seam" (bmi_conv1x1_seam_fwd: cin -> cout with
    residual and ReLU, then cout -> cn)."""
    cin: int
    cout: int
    H: int
    W: int
    k: int = 3
    stride: int = 1
    pad: int = 1
    n: int = 3
    in_mod: int = 0          # 0: n
    res_mod: int = 0         # 0: n
    scale: bool = True
    bias: bool = True
    res: bool = False
    relu: bool = True
    site: tuple = None       # None | ("elem", p) | ("chan", p) | ("msk",)
    batch: int = 0           # images per Monte-Carlo sample (0: n)
    entry: str = "conv"
    cout_b: int = 0
    cin2: int = 0
    cn: int = 0
    seed: int = 1

    @property
    def ho(self):
        return (self.H + 2 * self.pad - self.k) // self.stride + 1

    @property
    def wo(self):
        return (self.W + 2 * self.pad - self.k) // self.stride + 1

    @property
    def id(self):
        s = f"{self.entry}-{self.cin}to{self.cout}" + (f"+{self.cout_b}" if self.cout_b else "") + (f"+sc{self.cin2}" if self.cin2 else "") + \
            (f"to{self.cn}" if self.cn else "") + f"-{self.H}x{self.W}-k{self.k}s{self.stride}p{self.pad}-n{self.n}"
        if self.in_mod:
            s += f"-in{self.in_mod}"
        if self.res:
            s += "-res" + (str(self.res_mod) if self.res_mod else "")
        s += ("" if self.scale else "-noscale") + ("" if self.bias else "-nobias") + ("" if self.relu else "-norelu")
        if self.site:
            s += "-" + "".join(str(v) for v in self.site) + (f"b{self.batch}" if self.batch else "")
        return s


def flavour_for(dtype):
    """bf16 holds 8 significant bits: the bounded weights keep abs(out) <= (24 * 2 + 4 + 4) * 4 = 224.  The other types hold the dense ones
    (fp16: 11 bits; the pairs and fp32: 16 and more) — `exact_reference` asserts it for every case."""
    return "bounded" if dtype == "bf16" else "dense"


def _ternary(rng, shape):
    return torch.from_numpy(rng.integers(-1, 2, size=shape).astype(np.float64))


def _weights(rng, cout, kvol, flavour, nnz=NNZ):
    """[cout, kvol] in {-1, 0, 1}; bounded: at most `nnz` nonzeros per output channel at positions drawn per channel."""
    if flavour == "dense":
        return _ternary(rng, (cout, kvol))
    w = np.zeros((cout, kvol))
    nnz = min(nnz, kvol)
    # channel c's first positions walk a permutation of all (ky, kx, cin), so every position is used by some channel wherever
    # cout * nnz >= kvol; the others are drawn per channel
    perm, f = rng.permutation(kvol), min(nnz, -(-kvol // cout))
    for c in range(cout):
        forced = perm[(c * f + np.arange(f)) % kvol]
        rest = np.setdiff1d(np.arange(kvol), forced)
        pos = np.concatenate([forced, rng.choice(rest, size=nnz - f, replace=False)])
        w[c, pos] = rng.choice([-1.0, 1.0], size=len(pos))
    return torch.from_numpy(w)


def _pool_size(case, n_imgs, macs_per_image):
    return int(max(1, min(n_imgs, POOL, POOL_MACS // max(1, macs_per_image))))


def site_dict(case, cout):
    if case.site is None:
        return None
    if case.site[0] == "msk":      # Masksembles rows over {0, 2}
        rows = (np.random.default_rng(1000 + case.seed).random((4, cout)) < 0.5).astype(np.float32) * 2.0
        return dict(kind=_lib.SITE_MASKSEMBLE, site_id=1, masks=rows)
    return dict(kind=_lib.SITE_ELEMENTWISE if case.site[0] == "elem" else _lib.SITE_CHANNEL, site_id=4, p=case.site[1])


@functools.lru_cache(maxsize=8)
def exact_operands(case, flavour, seed=None):
    """float64 CPU operands of `case`: dict with x [n_in, H, W, Cin] (images drawn by index from a pool of at most 64), w [Cout, k, k, Cin],
    scale / bias [Cout] or None, res [n_res, Ho, Wo, Cout] or None, site (gpu_helpers form) or None; the pools and index lists the
    reference is computed from; and the second operand set of the pair / shortcut / seam entries."""
    rng = np.random.default_rng(case.seed if seed is None else seed)
    c = case
    n_in = c.in_mod or c.n
    kvol = c.k * c.k * c.cin
    cout_all = c.cout + c.cout_b
    o = dict(flavour=flavour)
    P = _pool_size(c, n_in, c.ho * c.wo * cout_all * kvol)
    o["x_pool"] = _ternary(rng, (P, c.H, c.W, c.cin))
    o["x_idx"] = torch.from_numpy(np.concatenate([np.arange(P), rng.integers(0, P, size=n_in - P)]))       # (every pool image is used)
    o["x"] = o["x_pool"][o["x_idx"]]
    seam = c.entry == "seam"
    # (the seam's wide tensor is the second conv's input: both convs thinned to 8 taps and scales <= 1 keep it within +-16 and the
    #  narrow output within +-132)
    o["w"] = _weights(rng, cout_all, kvol, "bounded" if seam else flavour, 8 if seam else NNZ).reshape(cout_all, c.k, c.k, c.cin)
    scales = [0.5, 1.0] if seam else [0.5, 1.0, 2.0]
    o["scale"] = torch.from_numpy(rng.choice(scales, size=cout_all)) if c.scale else None
    o["bias"] = torch.from_numpy(rng.integers(-4, 5, size=cout_all).astype(np.float64)) if c.bias else None
    o["res"] = None
    if c.res:
        n_res = c.res_mod or c.n
        Pr = min(n_res, POOL)
        pool = torch.from_numpy(rng.integers(-4, 5, size=(Pr, c.ho, c.wo, c.cout)).astype(np.float64))
        o["res"] = pool[torch.from_numpy(rng.integers(0, Pr, size=n_res))] if n_res > Pr else pool
    o["site"] = site_dict(c, c.cout)
    if c.entry == "shortcut":
        P2 = _pool_size(c, c.n, 4 * c.H * c.W * c.cin2)
        o["x2_pool"] = _ternary(rng, (P2, 2 * c.H, 2 * c.W, c.cin2))
        o["x2_idx"] = torch.from_numpy(rng.integers(0, P2, size=c.n)) if c.n > P2 else torch.arange(c.n)
        o["x2"] = o["x2_pool"][o["x2_idx"]]
        o["w2"] = _weights(rng, c.cout, c.cin2, "bounded", 8)
    if seam:
        o["w1"] = _weights(rng, c.cn, c.cout, "bounded", 8).reshape(c.cn, 1, 1, c.cout)
        o["scale1"] = torch.from_numpy(rng.choice(scales, size=c.cn))
        o["bias1"] = torch.from_numpy(rng.integers(-4, 5, size=c.cn).astype(np.float64))
    return o


def conv64(x_nhwc, w_okkc, stride, pad):
    """float64 conv as unfold + GEMM (torch's own float64 conv is several times slower): NHWC in, NCHW out."""
    n, H, W, cin = x_nhwc.shape
    cout, k = w_okkc.shape[0], w_okkc.shape[1]
    ho, wo = (H + 2 * pad - k) // stride + 1, (W + 2 * pad - k) // stride + 1
    wm = w_okkc.permute(0, 3, 1, 2).reshape(cout, -1).double()        # unfold's K order: (cin, ky, kx)
    out = torch.empty(n, cout, ho, wo, dtype=torch.float64)
    step = max(1, int(2.5e7 // max(1, cin * k * k * ho * wo)))
    for i in range(0, n, step):
        cols = F.unfold(x_nhwc[i:i + step].permute(0, 3, 1, 2).double(), k, padding=pad, stride=stride)
        out[i:i + step] = (wm @ cols).reshape(-1, cout, ho, wo)
    return out


def roundtrip(y, dtype):
    """y (float64) after a cast to the engine's output type and back."""
    if dtype in ("f16", "bf16"):
        return y.to(T16[dtype]).double()
    if dtype == "f32":
        return y.float().double()
    hi = y.float().to(T16[dtype])
    return hi.double() + (y.float() - hi.float()).to(T16[dtype]).double()


def _site_mult(site, n, batch, cout, ho, wo):
    if site is None:
        return None
    B = batch or n
    return gh.folded_site_mask(site, B, cout, ho, wo, -(-n // B), T0, SEED, CNT0)[:n].double()


def _finish(acc, scale, bias, res, res_mod, relu, mult):
    """conv_epilogue.h's order (epilogue_quad): BN scale, bias, residual row n % res_mod, ReLU, then the site multiplier."""
    n = acc.shape[0]
    y = acc
    if scale is not None:
        y = y * scale[None, :, None, None]
    if bias is not None:
        y = y + bias[None, :, None, None]
    if res is not None:
        y = y + res.permute(0, 3, 1, 2)[torch.arange(n) % res_mod]
    if relu:
        y = torch.relu(y)
    if mult is not None:
        y = y * mult
    return y


def _exact(y, dtype, what):
    assert torch.equal(roundtrip(y, dtype), y), f"{what}: the reference is not representable in {dtype}"
    return y.permute(0, 2, 3, 1).contiguous()


def _acc_ok(acc, kvol, xmax=1):
    # every partial sum, in any order, is bounded by the number of products times the largest product
    assert float(acc.abs().max()) < 2 ** 24 and kvol * xmax < 2 ** 24


@functools.lru_cache(maxsize=2)
def _reference64(case, flavour, seed):
    """float64 NCHW result(s) of `case` (cached: the option sets and dtypes of one case follow each other in the parameter lists)."""
    c = case
    o = exact_operands(c, flavour, seed)
    n_in = c.in_mod or c.n
    img = torch.arange(c.n) % n_in
    acc_pool = conv64(o["x_pool"], o["w"], c.stride, c.pad)
    _acc_ok(acc_pool, c.k * c.k * c.cin)
    acc = acc_pool[o["x_idx"][img]]
    if c.entry == "conv":
        mult = _site_mult(o["site"], c.n, c.batch, c.cout, c.ho, c.wo)
        return [_finish(acc, o["scale"], o["bias"], o["res"], c.res_mod or c.n, c.relu, mult)]
    if c.entry == "pair":
        y = _finish(acc, o["scale"], o["bias"], None, 1, c.relu, None)
        return [y[:, :c.cout], y[:, c.cout:]]
    if c.entry == "shortcut":
        a2 = conv64(o["x2_pool"], o["w2"].reshape(c.cout, 1, 1, c.cin2), 2, 0)
        _acc_ok(a2, c.cin2)
        return [_finish(acc + a2[o["x2_idx"]], None, o["bias"], None, 1, c.relu, None)]
    assert c.entry == "seam"
    wide = _finish(acc, o["scale"], o["bias"], o["res"], c.n, True, None)
    acc1 = conv64(wide.permute(0, 2, 3, 1), o["w1"], 1, 0)
    _acc_ok(acc1, c.cout, float(wide.abs().max()))
    return [wide, _finish(acc1, o["scale1"], o["bias1"], None, 1, c.relu, None)]


def exact_reference(case, dtype, flavour=None, seed=None):
    """float64 NHWC reference(s) of `case` for the engine dtype: a list with one tensor per output of the entry point.  Asserts that
    abs(acc) < 2^24 everywhere and that every result survives a cast to the output type and back — properties of the operands, not of a
    kernel, that make a bit-for-bit comparison legitimate."""
    return [_exact(y, dtype, case.id) for y in _reference64(case, flavour or flavour_for(dtype), seed)]


# ---- guarded allocations ----------------------------------------------------------------------------------------------------------
class Guarded:
    """`body` (a view shaped like the tensor) in the middle of one allocation whose two flanks hold `fill` (NaN; a byte pattern for integer
    tensors).  Each flank covers at least 256 pixels x the channels of a pixel and at least one image, rounded up to whole 512-byte blocks
    so the body keeps the allocator's alignment."""

    def __init__(self, shape, dtype, device, pixel_elems, image_elems, fill=float("nan")):
        numel = int(np.prod(shape))
        self.flank = -(-max(256 * pixel_elems, image_elems, 256) // 256) * 256
        self.fill = fill
        self.buf = torch.full((2 * self.flank + numel,), fill, dtype=dtype, device=device)
        self.body = self.buf[self.flank:self.flank + numel].view(shape)

    def flanks_intact(self):
        lo, hi = self.buf[:self.flank], self.buf[self.flank + self.body.numel():]
        if isinstance(self.fill, float):
            return bool(torch.isnan(lo).all()) and bool(torch.isnan(hi).all())
        return bool((lo == self.fill).all()) and bool((hi == self.fill).all())


def guarded(t, device=None, fill=float("nan")):
    """A copy of `t` (leading dimension = images, then pixels) between two flanks; `guarded_like` below for an output."""
    g = guarded_like(t.shape, t.dtype, device or t.device, fill)
    g.body.copy_(t)
    return g


def guarded_like(shape, dtype, device, fill=float("nan")):
    shape = tuple(int(s) for s in shape)
    image = int(np.prod(shape[1:])) if len(shape) > 1 else 1
    pixels = int(np.prod(shape[1:3])) if len(shape) > 3 else 1
    return Guarded(shape, dtype, device, image // max(1, pixels), image, fill)


# ---- launches ---------------------------------------------------------------------------------------------------------------------
def _act(t, dtype, dev):
    """an activation tensor in the engine's layout: 16-bit NHWC, fp32 NHWC, or the split engines' pair32."""
    if t is None:
        return None
    if dtype in ("f16", "bf16"):
        return guarded(t.to(T16[dtype]), dev)
    if dtype == "f32":
        return guarded(t.float(), dev)
    return guarded(gh.pair32_encode(t.float(), T16[dtype]), dev)


def _wgt(w, dtype, dev):
    """weights [Cout, ...]: 16-bit, fp32, or the split engines' head / tail planes [2, Cout, ...] (tests/test_split_engine.py split_planes)."""
    if dtype in ("f16", "bf16"):
        return guarded(w.to(T16[dtype]), dev)
    if dtype == "f32":
        return guarded(w.float(), dev)
    hi = w.float().to(T16[dtype])
    return guarded(torch.stack([hi, (w.float() - hi.float()).to(T16[dtype])]).contiguous(), dev)


def _vec(v, dev):
    return guarded(v.float(), dev) if v is not None else None


def _out(n, ho, wo, c, dtype, dev):
    if dtype in ("f16", "bf16"):
        return guarded_like((n, ho, wo, c), T16[dtype], dev)
    if dtype == "f32":
        return guarded_like((n, ho, wo, c), torch.float32, dev)
    return guarded_like((n, ho, wo, c // 32, 2, 32), T16[dtype], dev)


def _decode(g, dtype):
    return (gh.pair32_decode(g.body) if dtype in ("f16x2", "bf16x3") else g.body.float()).double().cpu()


def _p(g):
    return gh.ptr(g.body) if g is not None else None


def run_exact(case, dtype, opts=None, flavour=None):
    """Launches `case` through its single-kernel entry point under the element type `dtype` and the kernel-selection options `opts`
    (every option restored afterwards).  Returns (rc, outputs, guards_ok): the decoded float64 NHWC outputs (still all-NaN where nothing
    was written) and whether every flank of every operand and output is untouched."""
    c, dev, lib = case, gh.DEV, _lib.lib()
    o = exact_operands(c, flavour or flavour_for(dtype))
    x, w = _act(o["x"], dtype, dev), _wgt(o["w"][:c.cout], dtype, dev)
    sc, bi = _vec(o["scale"][:c.cout] if c.scale else None, dev), _vec(o["bias"][:c.cout] if c.bias else None, dev)
    res = _act(o["res"], dtype, dev)
    outs = [_out(c.n, c.ho, c.wo, c.cout, dtype, dev)]
    held = [x, w, sc, bi, res]
    keep = []
    n_in = c.in_mod or c.n
    with options(unit_entry_dtype=_lib.DTYPES[dtype], **(opts or {})):
        if c.entry == "conv":
            s = gh.site_struct(o["site"], keep)
            rc = lib.bmi_conv_igemm_fwd(_p(x), None, 1.0, _p(w), _p(sc), _p(bi), _p(res), _p(outs[0]), c.n, n_in, (c.res_mod or c.n) if c.res else 1,
                                        c.H, c.W, c.cin, c.cout, c.k, c.stride, c.pad, int(c.relu), C.byref(s) if s is not None else None,
                                        c.batch or c.n, T0, SEED, CNT0, gh.stream())
        elif c.entry == "pair":
            wb, sb, bb = _wgt(o["w"][c.cout:], dtype, dev), _vec(o["scale"][c.cout:], dev), _vec(o["bias"][c.cout:], dev)
            outs.append(_out(c.n, c.ho, c.wo, c.cout_b, dtype, dev))
            held += [wb, sb, bb]
            rc = lib.bmi_conv_pair_fwd(_p(x), _p(w), _p(sc), _p(bi), _p(outs[0]), _p(wb), _p(sb), _p(bb), _p(outs[1]), c.n, n_in, c.H, c.W, c.cin,
                                       c.cout, c.cout_b, c.k, c.stride, c.pad, int(c.relu), gh.stream())
        elif c.entry == "shortcut":
            x2, w2 = _act(o["x2"], dtype, dev), _wgt(o["w2"], dtype, dev)
            held += [x2, w2]
            rc = lib.bmi_conv3x3_shortcut_fwd(_p(x), _p(w), _p(x2), _p(w2), _p(bi), _p(outs[0]), c.n, c.H, c.W, c.cin, c.cout, c.cin2, int(c.relu),
                                              gh.stream())
        else:
            w1, s1, b1 = _wgt(o["w1"], dtype, dev), _vec(o["scale1"], dev), _vec(o["bias1"], dev)
            outs.append(_out(c.n, c.ho, c.wo, c.cn, dtype, dev))
            held += [w1, s1, b1]
            rc = lib.bmi_conv1x1_seam_fwd(_p(x), _p(w), _p(sc), _p(bi), _p(res), _p(outs[0]), _p(w1), _p(s1), _p(b1), _p(outs[1]), c.n, c.H, c.W, c.cin,
                                          c.cout, c.cn, int(c.relu), gh.stream())
        torch.cuda.synchronize()
    guards_ok = all(g.flanks_intact() for g in held + outs if g is not None)
    return rc, [_decode(g, dtype) for g in outs], guards_ok


def check_exact(case, dtype, expect, opts=None):
    """The one assertion of the GPU groups.  expect "ok": BMI_OK, every output equal to the reference bit for bit (so no NaN: every element
    written, no consumed read from a flank), flanks untouched.  expect "declined": BMI_ERR_UNSUPPORTED and every output still all-NaN."""
    refs = exact_reference(case, dtype)
    rc, outs, guards_ok = run_exact(case, dtype, opts)
    assert guards_ok, f"{case.id} {dtype} {opts}: a flank was written"
    if expect == "declined":
        assert rc == UNSUPPORTED, f"{case.id} {dtype} {opts}: rc = {rc}, expected a decline"
        assert all(bool(torch.isnan(t).all()) for t in outs), f"{case.id} {dtype}: a declined launch wrote to its output"
        return
    assert rc == _lib.BMI_OK, f"{case.id} {dtype} {opts}: rc = {rc}"
    for i, (got, ref) in enumerate(zip(outs, refs)):
        if not torch.equal(got, ref):
            bad = (got != ref) | torch.isnan(got)
            idx = bad.nonzero()
            raise AssertionError(f"{case.id} {dtype} {opts} output {i}: {int(bad.sum())} of {bad.numel()} elements differ ({int(torch.isnan(got).sum())} NaN); "
                                 f"first at (n, y, x, c) = {idx[0].tolist()}: got {float(got[tuple(idx[0])])}, want {float(ref[tuple(idx[0])])}; "
                                 f"last at {idx[-1].tolist()}")
