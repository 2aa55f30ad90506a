"""Host side of the MI355X MCD engine: compiles a model of ``bayesnn_fpga_amd.models`` into the
C-ABI graph (include/bayesnn_fpga_amd.h), owns the device buffers, and drives the library.

PyTorch is plumbing here (device memory, streams, ``torch.distributed``); all arithmetic of the
path runs in ``libbayesnn_fpga_amd.so``.  What this replaces in the reference:

* ``GraphBuilder``       — the op sequence of ``ResNet18MCEarlyExit.forward``
                           (SA/models/resnet18/resnet18.py:302-346; single-exit :246-258, :195-204),
                           with eval-mode BatchNorm folded to per-channel scale/bias and the
                           stochastic layers turned into *sites* numbered in call order
                           (SURVEY.md Appendix C).
* ``MCDEngine.predict``  — ``FullAnalysis._get_output`` (SA/train/results_analyzer.py:236-270): T passes,
                           per-exit softmax, float64 mean over T (+ build-defined variance).
"""
import ctypes as C
import os
from typing import NamedTuple, Optional

import numpy as np
import torch
from torch import nn

from . import _lib
from .utils import Masksembles1D, Masksembles2D

DEFAULT_CHUNK_IMAGES = 25600      # image-samples folded into one suffix launch (tuned on MI355X)
DEFAULT_CHUNK_SAMPLES_MAX = 128   # ... but never more than this many samples (the workspace is sized for a full chunk)
DEFAULT_ADAPTIVE_T_STEP = 25      # samples per step of predict_adaptive (never more than the planned chunk): a smaller step stops images
                                  # sooner but runs smaller launches and one more host sync per step.  Headline model, B = 250, T_max = 100,
                                  # SEM threshold at the median of the first step's (tools/adaptive_bench.py, MI355X): t_step 10 / 20 / 25 /
                                  # 50 -> 10.5 / 10.1 / 10.4 / 11.6 ms per batch (fixed T = 100: 22.1 ms); 20 and 25 are within noise, 25
                                  # splits T = 100 into four steps


def _is_site(m):
    return isinstance(m, (nn.Dropout, Masksembles1D, Masksembles2D))


def fold_bn(bn, conv_bias=None):
    """eval-mode BatchNorm2d -> (scale, bias) fp32:  y = conv * scale + bias."""
    with torch.no_grad():
        scale = bn.weight.double() / torch.sqrt(bn.running_var.double() + bn.eps)
        bias = bn.bias.double() - bn.running_mean.double() * scale
        if conv_bias is not None:
            bias = bias + conv_bias.double() * scale
    return scale.float(), bias.float()


class GraphBuilder:
    """Collects tensors / ops / device-resident weights for one model on one device."""

    def __init__(self, device, dtype="f16"):
        if dtype not in _lib.DTYPES:
            raise ValueError(f"dtype must be 'f16', 'bf16', 'f32' (the exact engine), 'f16x2' or 'bf16x3' (the split engines), got {dtype!r}")
        self.device = device
        self.dtype = dtype
        # conv weights: the engine's 16-bit type, fp32 (exact engine), or 16-bit head + tail planes (split engines: conv_weight below)
        self.act_dtype = {"f16": torch.float16, "bf16": torch.bfloat16, "f32": torch.float32, "f16x2": torch.float16, "bf16x3": torch.bfloat16}[dtype]
        self.tensors = []          # (h, w, c)
        self.ops = []              # dicts
        self.keep = []             # device tensors that must outlive the engine
        self.site_count = 0

    def tensor(self, h, w, c):
        self.tensors.append((int(h), int(w), int(c)))
        return len(self.tensors) - 1

    def dev(self, t, dtype):
        d = t.detach().to(device=self.device, dtype=dtype).contiguous()
        self.keep.append(d)
        return d

    def conv_weight(self, w, lift=None):
        """Device copy of a conv weight [Cout][ky][kx][Cin] in the engine's layout.  Split engines (BMI_DTYPE_F16X2 / BF16X3): the 16-bit
        head and tail planes [2][Cout][ky][kx][Cin], hi = rn16(w), lo = rn16(w - hi) — split once here, csrc/conv_split.hip reads both.
        ``lift`` [Cout] (``channel_lift``): the weights of output channel c are multiplied by the power of two lift[c] BEFORE they are
        rounded / split — exact — and the caller folds 1 / lift[c] into the channel's epilogue scale."""
        w32 = w.detach().float()
        if lift is not None:
            w32 = w32 * lift.to(w32.device).reshape((-1,) + (1,) * (w32.dim() - 1))
        if self.dtype not in ("f16x2", "bf16x3"):
            return self.dev(w32, self.act_dtype)
        hi = w32.to(self.act_dtype)
        lo = (w32 - hi.float()).to(self.act_dtype)
        return self.dev(torch.stack([hi, lo]), self.act_dtype)

    def channel_lift(self, *weights):
        """Per-output-channel power of two 2^k that brings max|w| of the channel (over ALL the given weights: a conv and its fused shortcut
        accumulate into one register) to [2^7, 2^8); None in the exact engine (fp32 weights).  Why: fp16 is denormal below 6.1e-5 and the
        split engines' fp16 TAIL rn16(w - hi) of any weight below 2^-3 is a subnormal (ulp 2^-24) — BN-folded conv weights of 1e-2 .. 1e-3
        would keep 15-18 of the 22 bits the split form is for, anything under 6e-8 nothing (round-5 advisor finding); the plain fp16 engine
        loses bits of every weight under 6.1e-5 the same way.  Lifted, every head and every tail that matters is a normal number; 2^-k goes
        into the fp32 epilogue scale — exact, and for weights that were normal numbers anyway bit for bit the unlifted result (a power of
        two commutes with every rounding on the way).  bf16 has fp32's exponent range: harmless there, one code path."""
        if self.dtype == "f32":
            return None
        amax = torch.stack([w.detach().float().abs().reshape(w.shape[0], -1).amax(dim=1) for w in weights]).amax(dim=0)
        k = 7 - torch.floor(torch.log2(amax.clamp_min(1e-30)))
        k = torch.where(amax > 0, k, torch.zeros_like(k)).clamp_(-8, 30)
        return torch.pow(2.0, k)

    def site(self, module, channelwise=False):
        """Allocates the next site id (call order) for a stochastic layer, or none."""
        if module is None:
            return None
        sid = self.site_count
        self.site_count += 1
        if channelwise:
            return dict(kind=_lib.SITE_CHANNEL, site_id=sid, p=float(module.p))
        if isinstance(module, (Masksembles1D, Masksembles2D)):
            masks = self.dev(module.masks, torch.float32)
            return dict(kind=_lib.SITE_MASKSEMBLE, site_id=sid, num_masks=module.n, masks=masks)
        return dict(kind=_lib.SITE_ELEMENTWISE, site_id=sid, p=float(module.p))

    def conv(self, x, conv, bn, relu, residual=-1, site=None, stem=False, shortcut=None, site_inner=False):
        """conv (+ folded BN) op.  ``shortcut=(x2, conv1x1, bn)`` fuses the BasicBlock downsample path into this
        conv as extra K-steps: both BN scales are folded into the fp16 weights, the biases are summed.
        ``site_inner``: the site sits between the conv and its BatchNorm (converter/pytorch rule):
        out = relu((conv*scale + scale*conv.bias) * mask + bn_shift)."""
        h, w, cin = self.tensors[x]
        k, s, p = conv.kernel_size[0], conv.stride[0], conv.padding[0]
        ho, wo = (h + 2 * p - k) // s + 1, (w + 2 * p - k) // s + 1
        out = self.tensor(ho, wo, conv.out_channels)
        if bn is not None:
            scale, bias = fold_bn(bn, conv.bias)
        else:
            scale = torch.ones(conv.out_channels)
            bias = conv.bias.detach().float() if conv.bias is not None else torch.zeros(conv.out_channels)
        bias_post = None
        if site_inner and site is not None:
            if bn is None or shortcut is not None:
                raise ValueError("an inner site needs a BatchNorm behind the conv and no fused shortcut")
            scale, shift = fold_bn(bn, None)
            bias_post = shift
            bias = scale * conv.bias.detach().float() if conv.bias is not None else torch.zeros_like(scale)
        wk = conv.weight.detach().permute(0, 2, 3, 1)          # [Cout][ky][kx][Cin]
        in2, w2dev = -1, None
        if shortcut is not None:
            x2, conv_s, bn_s = shortcut
            s_scale, s_bias = fold_bn(bn_s, conv_s.bias)
            wk = wk.float() * scale[:, None, None, None]
            w2 = conv_s.weight.detach().float()[:, :, 0, 0] * s_scale[:, None]       # [Cout][Cin2]
            # (the 16-bit engines' shortcut-carrying kernels take no scale beside in2 — both BN scales are in the weights — so no lift there)
            lift = self.channel_lift(wk, w2) if self.dtype in ("f16x2", "bf16x3") else None
            w2dev = self.conv_weight(w2, lift)                                         # (split engines: head / tail planes)
            bias = bias + s_bias
            scale = None if lift is None else (1.0 / lift).to(bias.device)
            in2 = x2
        else:
            lift = None if stem else self.channel_lift(wk)
            if lift is not None:
                scale = scale / lift.to(scale.device)
        wdev = self.dev(wk, torch.float32) if stem else self.conv_weight(wk, lift)
        self.ops.append(dict(kind=_lib.OP_STEM if stem else _lib.OP_CONV, in_=x, out=out, residual=residual, ksize=k,
                             stride=s, pad=p, relu=int(relu), weight=wdev, in2=in2, weight2=w2dev,
                             scale=self.dev(scale, torch.float32) if scale is not None else None,
                             bias=self.dev(bias, torch.float32), site=site,
                             bias_post=self.dev(bias_post, torch.float32) if bias_post is not None else None,
                             site_pos=_lib.SITE_POS_INNER if bias_post is not None else _lib.SITE_POS_OUTER))
        return out

    def mask(self, x, site):
        h, w, c = self.tensors[x]
        out = self.tensor(h, w, c)
        self.ops.append(dict(kind=_lib.OP_MASK, in_=x, out=out, residual=-1, site=site))
        return out

    def maxpool(self, x):
        h, w, c = self.tensors[x]
        out = self.tensor(h // 2, w // 2, c)
        self.ops.append(dict(kind=_lib.OP_MAXPOOL, in_=x, out=out, residual=-1))
        return out

    def dense(self, x, linear, relu, site=None):
        """Hidden fully-connected layer on a flattened [N,1,1,C] tensor, fp32 weights / accumulation / output
        (BMI_OP_DENSE: as a 1x1 fp16 conv the two VGG-11 dense layers pushed the predictive mean past 1e-3 at B=250)."""
        h, w, cin = self.tensors[x]
        if (h, w) != (1, 1) or cin != linear.in_features:
            raise ValueError("dense layers run on flattened [N,1,1,C] tensors")
        if cin % 32 or linear.out_features % 64:
            # (zero-padding would move the Philox element index of a site on the padded tensor — index = row * C + c — away from
            #  the reference's; the converter puts a site behind EVERY Linear)
            raise TypeError(f"hidden Linear({cin}, {linear.out_features}): the accelerated path takes in_features % 32 == 0 and "
                            "out_features % 64 == 0")
        out = self.tensor(1, 1, linear.out_features)
        self.ops.append(dict(kind=_lib.OP_DENSE, in_=x, out=out, residual=-1, relu=int(relu),
                             weight=self.dev(linear.weight, torch.float32), bias=self.dev(linear.bias, torch.float32), site=site))
        return out

    def head(self, x, linear, exit_index, site=None, site_on_logits=False):
        """relu -> global average pool -> [site] -> Linear -> [site on the logits] -> softmax."""
        c_in = self.tensors[x][2]
        if linear.in_features != c_in:
            raise ValueError(f"classifier expects {linear.in_features} features, pooled tensor has {c_in}")
        if c_in % 32:
            raise TypeError(f"classifier Linear({c_in}, {linear.out_features}): the accelerated path takes in_features % 32 == 0")
        cpad = (linear.out_features + 31) // 32 * 32
        w = torch.zeros(cpad, c_in)
        w[:linear.out_features] = linear.weight.detach().float()
        self.ops.append(dict(kind=_lib.OP_HEAD, in_=x, out=exit_index, residual=-1,
                             weight=self.dev(w, torch.float32), bias=self.dev(linear.bias, torch.float32), site=site,
                             site_pos=_lib.SITE_POS_INNER if (site_on_logits and site) else _lib.SITE_POS_OUTER))


def _unwrap(module):
    """Sequential(inner, site) wrappers made by the dropout-insertion rules -> (inner, site | None)."""
    if isinstance(module, nn.Sequential) and len(module) == 2 and _is_site(module[1]):
        return module[0], module[1]
    return module, None


def _can_fuse_shortcut(t_in, blk, dtype="f16"):
    """The 1x1 strided downsample conv rides along in the 3x3 patch kernel when that kernel takes conv2
    (16x16 / 8x8 / 4x4 maps, Cout % 128 == 0) and the block input has a multiple of 64 channels.
    BMI_FUSE_SHORTCUT=0 keeps the separate launch + residual (A/B, tests); the exact engine never fuses (the fusion folds
    the BN scales into the 16-bit weights: a speed feature)."""
    if os.environ.get("BMI_FUSE_SHORTCUT", "1") == "0" or dtype == "f32":
        return False
    h, w, c = t_in
    ds = blk.downsample[0]
    if dtype in _lib.FP32_ACT_DTYPES:       # the split engines: extra K-steps of the generic kernel, whatever the map (csrc/conv_split.hip)
        return c % 32 == 0 and ds.in_channels % 32 == 0 and ds.kernel_size == (1, 1) and ds.bias is None and ds.padding == (0, 0)
    return ((h, w) in ((16, 16), (8, 8), (4, 4)) and blk.conv2.out_channels % 128 == 0 and c % 64 == 0
            and ds.in_channels % 64 == 0 and ds.kernel_size == (1, 1) and ds.stride == (2, 2) and ds.bias is None)


def _converted(m):
    """``(layer, wrapper | None)`` for a layer the torch "nn2bnn" converter may have wrapped (converter/pytorch/Dropouts.py:
    BayesianDropout* own the layer as ``.layer`` and drop its OUTPUT in every mode)."""
    if m is not None and type(m).__name__.startswith("BayesianDropout") and hasattr(m, "layer"):
        return m.layer, m
    return m, None


def build_resnet_graph(model, g):
    """Op sequence of the ResNet family forwards (reference resnet18.py:302-346 / :246-258 / :195-204).

    Also compiles a mirror that went through the converter (``nn2bnn._convert_model``: every Conv2d wrapped in
    BayesianDropout2D, every Linear in BayesianDropout — Hardware_Artifact/converter/pytorch/nn2bnn.py:32-45): a wrapped conv
    carries a per-(image, channel) site BETWEEN the conv and its BatchNorm (an inner site of the C ABI), a wrapped Linear an
    elementwise site on its logits; site ids follow the CALL order of the reference forward (BasicBlock.forward :32-48: conv1,
    conv2, then the downsample conv), and a shortcut conv that carries a site keeps its own launch."""
    x = g.tensor(32, 32, 3)                                   # tensor 0: network input (fp32 NCHW)
    stem, stem_w = _converted(model.conv1)
    x = g.conv(x, stem, model.bn1, relu=False, stem=True,       # no ReLU after the stem (:303)
               site=g.site(stem_w, channelwise=True), site_inner=stem_w is not None)
    multi = getattr(model, "multi_exit", True)
    dropout_exit = getattr(model, "dropout_exit", False)
    exit_sites = {1: "exit1_dropout", 2: "exit2_dropout", 3: "exit3_dropout"}

    def head(y, linear, index, feature_site_module):
        lin, lin_w = _converted(linear)
        if lin_w is not None and feature_site_module is not None:
            raise TypeError("a converted classifier (dropout on the logits) on top of an exit dropout is not on the accelerated path")
        if lin_w is not None:
            g.head(y, lin, index, site=g.site(lin_w), site_on_logits=True)
        else:
            g.head(y, lin, index, site=g.site(feature_site_module))

    for si in range(1, 5):
        stage, stage_site = _unwrap(getattr(model, f"layer{si}"))
        blocks = list(stage)
        for bi, blk in enumerate(blocks):
            blk, blk_site = _unwrap(blk)
            site_mod = blk_site if blk_site is not None else (stage_site if bi == len(blocks) - 1 else None)
            c1, w1 = _converted(blk.conv1)
            c2, w2 = _converted(blk.conv2)
            ds, wd = _converted(blk.downsample[0]) if blk.downsample is not None else (None, None)
            if w2 is not None and site_mod is not None:
                raise TypeError("a converted conv (site before its BatchNorm) under a block / stage dropout is not on the accelerated path")
            a = g.conv(x, c1, blk.bn1, relu=True, site=g.site(w1, channelwise=True), site_inner=w1 is not None)
            # site ids follow call order: a block's site is allocated when the block finishes; conv2's before the shortcut's
            site2 = g.site(w2, channelwise=True) if w2 is not None else g.site(site_mod)
            if ds is not None and wd is None and w2 is None and _can_fuse_shortcut(g.tensors[a], blk, g.dtype):
                x = g.conv(a, c2, blk.bn2, relu=True, site=site2, shortcut=(x, ds, blk.downsample[1]))
            else:
                res = x
                if ds is not None:
                    res = g.conv(x, ds, blk.downsample[1], relu=False, site=g.site(wd, channelwise=True), site_inner=wd is not None)
                x = g.conv(a, c2, blk.bn2, relu=True, residual=res, site=site2, site_inner=w2 is not None)
        if multi and si < 4:
            # exit head si: relu -> conv s2 -> bn chain, relu, avg-pool, [exit dropout], linear
            # (F.relu on a stage output is idempotent: it is already >= 0 and masks keep the sign)
            y = x
            n_conv = 4 - si
            for j in range(1, n_conv + 1):
                ec, ew = _converted(getattr(model, f"ex{si}conv{j}"))
                y = g.conv(y, ec, getattr(model, f"ex{si}bn{j}"), relu=True, site=g.site(ew, channelwise=True), site_inner=ew is not None)
            sm = getattr(model, exit_sites[si], None) if dropout_exit else None
            head(y, getattr(model, f"ex{si}linear"), si - 1, sm)
    sm = getattr(model, "exit_dropout", None) if dropout_exit else None
    head(x, model.linear, (model_exits(model) - 1), sm)


def model_exits(model):
    """Number of logits tensors the reference forward returns (4 multi-exit, 1 single-exit)."""
    if hasattr(model, "build_graph"):
        return int(model.n_exits)
    if getattr(model, "family", "") == "vgg":
        return 5 if getattr(model, "multi_exit", True) else 1
    return 4 if getattr(model, "multi_exit", True) else 1


def check_stop_on(stop_on, ensemble):
    """``stop_on`` of accumulate_adaptive / predict_adaptive: "exit" or "ensemble", the latter only with ``ensemble=True`` (host only)."""
    if stop_on not in _lib.STOP_ON:
        raise ValueError(f"stop_on must be one of {sorted(_lib.STOP_ON)}, got {stop_on!r}")
    if stop_on == "ensemble" and not ensemble:
        raise ValueError('stop_on="ensemble" needs ensemble=True: the rule reads the exit-ensemble sums')


def check_temperature(tau, n_exits):
    """``tau`` as a plain list of ``n_exits`` Python floats, or None (off): a scalar stands for every exit; raises ValueError for a wrong
    count, a non-finite or a non-positive entry, or one whose float32 value (what the device is given) is not finite and positive."""
    if tau is None:
        return None
    raw = np.asarray(tau.detach().cpu() if isinstance(tau, torch.Tensor) else tau, dtype=np.float64)
    vals = np.repeat(raw.reshape(-1), n_exits) if raw.ndim == 0 else raw.reshape(-1)
    if vals.size != n_exits:
        raise ValueError(f"temperature: expected one value per exit ({n_exits}), got {vals.size}")
    with np.errstate(over="ignore", divide="ignore"):
        f32 = vals.astype(np.float32)
        inv = (1.0 / f32.astype(np.float64)).astype(np.float32)
    if not (np.all(np.isfinite(vals)) and np.all(vals > 0) and np.all(np.isfinite(f32)) and np.all(f32 > 0) and np.all(np.isfinite(inv)) and np.all(inv > 0)):
        raise ValueError(f"temperature: every entry must be finite and > 0 (in float32, and its reciprocal too), got {vals.tolist()}")
    return [float(v) for v in vals]


def check_ensemble_weights(w, n_exits):
    """The weights of the exit ensembles as a float64 array [E, E] (row e: the weights of the ensemble of exits 0..e), or None (off: the
    equal-weight mean).  ``w``: None, an [E] vector — one non-negative weight per exit, expanded as W[e][i] = w_i / fsum(w[:e+1]), every
    prefix sum > 0 — or an [E, E] matrix.  Raises ValueError for any other shape, a negative or non-finite entry, a nonzero entry above the
    diagonal, or a row whose (exactly rounded) sum is further than 1e-12 from 1.  Host only."""
    if w is None:
        return None
    import math
    E = int(n_exits)
    raw = np.array(w.detach().cpu().numpy() if isinstance(w, torch.Tensor) else w, dtype=np.float64)
    if not np.all(np.isfinite(raw)) or np.any(raw < 0):
        raise ValueError("ensemble weights: every entry must be finite and >= 0")
    if raw.shape == (E,):
        W = np.zeros((E, E), dtype=np.float64)
        for e in range(E):
            tot = math.fsum(raw[:e + 1])
            if not tot > 0:
                raise ValueError(f"ensemble weights: the weights of exits 0..{e} sum to {tot}, every prefix sum must be > 0")
            W[e, :e + 1] = raw[:e + 1] / tot
    elif raw.shape == (E, E):
        W = np.ascontiguousarray(raw)
    else:
        raise ValueError(f"ensemble weights: expected [{E}] or [{E}, {E}] for {E} exits, got {list(raw.shape)}")
    if np.any(np.triu(W, 1) != 0):
        raise ValueError("ensemble weights: W[e][i] must be 0 for i > e (the ensemble of exits 0..e has no later member)")
    sums = [math.fsum(row) for row in W]
    if not all(abs(v - 1.0) <= 1e-12 for v in sums):
        raise ValueError(f"ensemble weights: every row must sum to 1 within 1e-12, got {sums}")
    return W


def _check_affine_map(what, name, weight, bias, n_exits, out_dim, tail):
    """The body of ``check_vector_scaling`` (``tail`` = (C,)) and ``check_matrix_scaling`` (``tail`` = (C, C)): ``weight`` as float32
    [E, *tail] and ``bias`` as float32 [E, C], C-contiguous, each also taken without the leading E (every exit) and ``bias`` None = zeros;
    (None, None) when ``weight`` is None.  ``what`` / ``name``: what the messages call the map and its first array."""
    if weight is None:
        if bias is not None:
            raise ValueError(f"{what}: a bias needs a {name}")
        return None, None
    E, Cd = int(n_exits), int(out_dim)
    out = []
    for name, v, tail in ((name, weight, tail), ("bias", bias, (Cd,))):
        if v is None:
            out.append(np.zeros((E,) + tail, dtype=np.float32))
            continue
        raw = np.asarray(v.detach().cpu().numpy() if isinstance(v, torch.Tensor) else v, dtype=np.float64)
        if raw.shape == tail:
            raw = np.broadcast_to(raw, (E,) + tail)
        elif raw.shape != (E,) + tail:
            raise ValueError(f"{what}: {name} must be {[E, *tail]} or {list(tail)} for {E} exits of {Cd} classes, got {list(raw.shape)}")
        with np.errstate(over="ignore"):
            f32 = np.ascontiguousarray(raw, dtype=np.float32)
        if not (np.all(np.isfinite(raw)) and np.all(np.isfinite(f32))):
            raise ValueError(f"{what}: every {name} value must be finite (in float32 too)")
        out.append(f32)
    return out[0], out[1]


def check_vector_scaling(scale, bias, n_exits, out_dim):
    """Vector scaling as two C-contiguous float32 arrays [E, C] (scale, bias), or (None, None) when ``scale`` is None (off).  ``scale`` / ``bias``:
    [E, C], or [C] for every exit; ``bias`` None = zeros.  Raises ValueError for any other shape, for a bias without a scale and for a value
    that is not finite (in float32, what the device is given).  No sign constraint.  Host only."""
    return _check_affine_map("vector scaling", "scale", scale, bias, n_exits, out_dim, (int(out_dim),))


def check_matrix_scaling(matrix, bias, n_exits, out_dim):
    """Matrix scaling as two C-contiguous float32 arrays (matrix [E, C, C] — row = output class —, bias [E, C]), or (None, None) when
    ``matrix`` is None (off).  ``matrix``: [E, C, C], or [C, C] for every exit; ``bias``: [E, C], or [C] for every exit, None = zeros.
    Raises ValueError for any other shape, for a bias without a matrix and for a value that is not finite (in float32, what the device
    is given).  No sign constraint.  Host only."""
    return _check_affine_map("matrix scaling", "matrix", matrix, bias, n_exits, out_dim, (int(out_dim),) * 2)


class CalibrationMap(NamedTuple):
    """What ``resolve_calibration_map`` returns: ``kind`` None (no map), "temperature", "vector" or "matrix", and the checked host values —
    ``tau`` (``check_temperature``'s list) for a temperature; ``weight`` (the scale [E, C] or the matrix [E, C, C]) and ``bias`` [E, C],
    float32, for the other two.  What a kind does not use is None."""
    kind: Optional[str] = None
    tau: Optional[list] = None
    weight: Optional[np.ndarray] = None
    bias: Optional[np.ndarray] = None


def resolve_calibration_map(tau=None, scale=None, bias=None, matrix=None, *, n_exits, out_dim, who):
    """THE rule of the calibration maps, for every caller that takes one (the engine and model setters, ``ensemble_moments``, ``vote_counts``,
    ``train.uncertainty.calibrated_logits``): at most one of ``tau`` (``check_temperature``), ``scale`` (``check_vector_scaling``, with
    ``bias``) and ``matrix`` (``check_matrix_scaling``, with ``bias``), checked by its own function and returned as a ``CalibrationMap``.
    ValueError — ``who`` names the caller — when two are given together or a bias comes alone, and whatever the check of the one that is
    given raises.  Host only."""
    given = [name for name, v in (("tau", tau), ("scale", scale), ("matrix", matrix)) if v is not None]
    if len(given) > 1:
        raise ValueError(f"{who}: {' and '.join(given)} were given together (one calibration map at a time)")
    if bias is not None and scale is None and matrix is None:
        raise ValueError(f"{who}: a bias needs a scale or a matrix")
    if matrix is not None:
        return CalibrationMap("matrix", None, *check_matrix_scaling(matrix, bias, n_exits, out_dim))
    if scale is not None:
        return CalibrationMap("vector", None, *check_vector_scaling(scale, bias, n_exits, out_dim))
    tau = check_temperature(tau, n_exits)
    return CalibrationMap(None if tau is None else "temperature", tau)


def vary_mask(vary, n_exits):
    """``vary`` of ensemble_nll_grid (an exit index, an iterable of indices, or None) as the bit mask bmi_nll_ensemble_temperature_grid
    takes; raises ValueError for an index outside [0, n_exits)."""
    idx = [] if vary is None else [int(vary)] if np.ndim(vary) == 0 else [int(i) for i in vary]
    if any(i < 0 or i >= n_exits for i in idx):
        raise ValueError(f"vary: exit indices must lie in [0, {n_exits}), got {idx}")
    mask = 0
    for i in idx:
        mask |= 1 << i
    return mask


def check_buffer(t, shape, dtype, device, name):
    """The one validation of a buffer whose pointer goes to the C ABI: ``t`` is a contiguous tensor of ``dtype`` and ``shape`` (None: any
    extent in that dimension) on ``device``; ``name`` is what the message calls it.  ValueError otherwise; returns ``t``."""
    ok = isinstance(t, torch.Tensor) and t.dim() == len(shape) and all(w is None or w == g for w, g in zip(shape, t.shape)) and \
        t.dtype == dtype and t.is_contiguous() and t.device == device
    if not ok:
        want = [("*" if w is None else w) for w in shape]
        got = f"{t.dtype} {list(t.shape)} on {t.device}{'' if t.is_contiguous() else ', not contiguous'}" if isinstance(t, torch.Tensor) else repr(t)
        raise ValueError(f"{name} must be a contiguous {dtype} tensor {want} on {device}, got {got}")
    return t


def _ptr(t):
    """The device address of a tensor for the C ABI, None for None."""
    return None if t is None else t.data_ptr()


def build_graph(model, device, dtype="f16"):
    g = GraphBuilder(device, dtype)
    fam = getattr(model, "family", None)
    if fam == "resnet":
        build_resnet_graph(model, g)
    elif fam == "vgg":
        from .models.vgg19.vgg19 import build_vgg_graph
        build_vgg_graph(model, g)
    elif hasattr(model, "build_graph"):
        model.build_graph(g)
    else:
        raise TypeError(f"{type(model).__name__} is not a bayesnn_fpga_amd model")
    return g


# the calibration maps of an engine, kind -> (what a message calls it, the MCDEngine setter that clears it, the C setter)
_MAPS = {"temperature": ("temperature", "set_temperature", "bmi_engine_set_temperature"),
         "vector": ("vector scaling", "set_vector_scaling", "bmi_engine_set_vector_scaling"),
         "matrix": ("matrix scaling", "set_matrix_scaling", "bmi_engine_set_matrix_scaling")}


class CompiledGraph:
    """Host-only half of the engine: graph -> C descriptors -> bmi_create / bmi_plan / bmi_query.
    Touches no GPU API (weights only need to be addressable), so it also runs on a CPU-only box."""

    def __init__(self, model, device, max_batch, chunk_samples=None, dtype="f16"):
        self.lib = _lib.lib()
        self.device = torch.device(device)
        self.n_exits = model_exits(model)
        self.out_dim = int(model.out_dim)
        self.dtype = dtype
        self.graph = build_graph(model, self.device, dtype)
        self.max_batch = int(max_batch)
        self.chunk_explicit = chunk_samples is not None
        if chunk_samples is None:
            chunk_samples = min(DEFAULT_CHUNK_SAMPLES_MAX, max(1, DEFAULT_CHUNK_IMAGES // self.max_batch))
        self.chunk_samples = int(chunk_samples)
        self._desc_keep = self._make_desc()
        self.handle = C.c_void_p()
        _lib.check(self.lib.bmi_create(C.byref(self._desc_keep[0]), C.byref(self.handle)), "bmi_create")
        ws = C.c_size_t()
        _lib.check(self.lib.bmi_plan(self.handle, self.max_batch, self.chunk_samples, C.byref(ws)), "bmi_plan")
        self.workspace_bytes = ws.value
        pm, sm, npo, nso = C.c_int64(), C.c_int64(), C.c_int32(), C.c_int32()
        _lib.check(self.lib.bmi_query(self.handle, C.byref(pm), C.byref(sm), C.byref(npo), C.byref(nso)), "bmi_query")
        self.prefix_macs, self.suffix_macs = pm.value, sm.value
        self.n_prefix_ops, self.n_suffix_ops = npo.value, nso.value
        # MACs that do not run in the MFMA conv kernels (bench.py's roofline accounting): the direct stem and the heads
        t = self.graph.tensors
        # whether the Philox seed reaches any kernel: Masksembles-only graphs (SA/utils.py: the masks are part of the state_dict) do not draw
        self.seed_matters = any((o.get("site") or {}).get("kind") in (_lib.SITE_ELEMENTWISE, _lib.SITE_CHANNEL) for o in self.graph.ops)
        self.stem_macs = sum(t[o["out"]][0] * t[o["out"]][1] * t[o["out"]][2] * 27 for o in self.graph.ops if o["kind"] == _lib.OP_STEM)
        self.head_macs = sum(t[o["in_"]][2] * self.out_dim for o in self.graph.ops if o["kind"] == _lib.OP_HEAD)
        self.dense_macs = sum(t[o["in_"]][2] * t[o["out"]][2] for o in self.graph.ops if o["kind"] == _lib.OP_DENSE)
        # per-exit temperature scaling: a model that carries one (EngineModelMixin.set_exit_temperature, train/calibration.py) hands it to
        # every engine built from it — model.engine(), BatchesInFlight, FullAnalysis, evaluate's pipes, the sharded walks, the "auto" calibration
        self.set_temperature(getattr(model, "exit_temperature", None))

    def set_temperature(self, tau):
        """One softmax temperature per exit (bmi_engine_set_temperature; host only): a scalar (every exit) or ``n_exits`` values, finite and
        > 0; ``None`` — or all ones — is off.  From the next launch on, every path through the fused head (predict, accumulate,
        predict_uncertainty, predict_with_exit, predict_early_exit, predict_adaptive, the moment sums of the sharded walks) computes softmax,
        mean, var and the entropies of ``logit * float32(1 / tau_e)``; ``logit_mean``, ``forward_once`` and ``forward_samples`` stay the raw
        logits and do not depend on it.  Off, the engine launches the untempered kernels: the bits of an engine that never had one.  A hipGraph
        captured earlier keeps the temperature it was captured with (``BatchesInFlight.set_temperature`` discards them)."""
        tau = check_temperature(tau, self.n_exits)
        if tau is None:
            rc = self.lib.bmi_engine_set_temperature(self.handle, None, 0)
        else:
            rc = self.lib.bmi_engine_set_temperature(self.handle, (C.c_float * self.n_exits)(*tau), self.n_exits)
        _lib.check(rc, "bmi_engine_set_temperature")

    @property
    def temperature(self):
        """The temperatures in force, a list of ``n_exits`` floats (ones when off)."""
        buf = (C.c_float * self.n_exits)()
        _lib.check(self.lib.bmi_engine_get_temperature(self.handle, buf, self.n_exits), "bmi_engine_get_temperature")
        return [float(v) for v in buf]

    def exit_stages(self, first_exit=1):
        """The stage plan of ``MCDEngine.predict_early_exit`` (bmi_query_exit_stages, host only): a list with one dict per decision stage,
        stage 0 holding every op up to exit ``first_exit``: prefix_macs (per image), suffix_macs (per image and sample), n_ops, and the
        prefix ops of the stage that run over the whole batch because their kernel has no row-table form (whole_batch_macs per image, also
        counted in prefix_macs; n_whole_batch_ops)."""
        first_exit = int(first_exit)
        if not 0 <= first_exit < self.n_exits:
            raise ValueError(f"first_exit must be in [0, {self.n_exits})")
        n = C.c_int32(0)
        _lib.check(self.lib.bmi_query_exit_stages(self.handle, first_exit, 0, C.byref(n), None, None, None, None, None), "bmi_query_exit_stages")
        k = n.value
        pm, sm, wm = (C.c_int64 * k)(), (C.c_int64 * k)(), (C.c_int64 * k)()
        no, nw = (C.c_int32 * k)(), (C.c_int32 * k)()
        _lib.check(self.lib.bmi_query_exit_stages(self.handle, first_exit, k, C.byref(n), pm, sm, no, wm, nw), "bmi_query_exit_stages")
        return [dict(prefix_macs=pm[i], suffix_macs=sm[i], n_ops=no[i], whole_batch_macs=wm[i], n_whole_batch_ops=nw[i]) for i in range(k)]

    def op_stages(self, first_exit=1):
        """The stage plan per op (bmi_query_op_stages): a list of (out, stage, whole_batch) in the engine's order, one entry per output of
        every op (a pair- or seam-fused op lists both); ``out`` is the tensor id, or -1 - the exit index for a head."""
        first_exit = int(first_exit)
        if not 0 <= first_exit < self.n_exits:
            raise ValueError(f"first_exit must be in [0, {self.n_exits})")
        n = C.c_int32(0)
        _lib.check(self.lib.bmi_query_op_stages(self.handle, first_exit, 0, C.byref(n), None, None, None), "bmi_query_op_stages")
        k = n.value
        out, st, wb = (C.c_int32 * k)(), (C.c_int32 * k)(), (C.c_int32 * k)()
        _lib.check(self.lib.bmi_query_op_stages(self.handle, first_exit, k, C.byref(n), out, st, wb), "bmi_query_op_stages")
        return [(out[i], st[i], bool(wb[i])) for i in range(k)]

    def _make_desc(self):
        g = self.graph
        tarr = (_lib.TensorDesc * len(g.tensors))(*[_lib.TensorDesc(*t) for t in g.tensors])
        oarr = (_lib.OpDesc * len(g.ops))()
        for i, op in enumerate(g.ops):
            d = oarr[i]
            d.kind, d.in_, d.out, d.residual = op["kind"], op["in_"], op["out"], op.get("residual", -1)
            d.ksize, d.stride, d.pad, d.relu = op.get("ksize", 0), op.get("stride", 0), op.get("pad", 0), op.get("relu", 0)
            d.in2 = op.get("in2", -1)
            d.site_pos = op.get("site_pos", _lib.SITE_POS_OUTER)
            for f in ("weight", "weight2", "scale", "bias", "bias_post"):
                t = op.get(f)
                setattr(d, f, t.data_ptr() if t is not None else None)
            s = op.get("site")
            if s:
                d.site = _lib.make_site(s["kind"], s["site_id"], s.get("p", 0.0), s.get("num_masks", 0),
                                        s["masks"].data_ptr() if "masks" in s else None)
            else:
                d.site = _lib.make_site()
        desc = _lib.ModelDesc(len(g.tensors), tarr, len(g.ops), oarr, self.n_exits, self.out_dim,
                              _lib.DTYPES[self.dtype])
        return (desc, tarr, oarr)

    def flops_per_batch(self, batch, T):
        """Executed-algorithmic FLOPs (prefix once + T x suffix), conv + linear only, 1 MAC = 2 FLOP."""
        return 2 * batch * (self.prefix_macs + T * self.suffix_macs)

    def conv_traffic_model(self, batch, T):
        """Algorithmic HBM bytes and launch count of the MFMA conv kernels for one batch x T samples: every conv reads
        its input (+ residual / shortcut input) and weights once and writes its output once, fp16.  A conv whose inputs
        are all deterministic runs once per batch (prefix), the others once per chunk of ``chunk_samples`` samples."""
        t, stoch = self.graph.tensors, set()
        chunks = -(-T // self.chunk_samples)
        total, launches = 0, 0
        for o in self.graph.ops:
            ins = [o["in_"]] + [o[k] for k in ("residual", "in2") if o.get(k, -1) is not None and o.get(k, -1) >= 0]
            det = not any(i in stoch for i in ins)
            if o["kind"] != _lib.OP_HEAD and (o.get("site") or not det):
                stoch.add(o["out"])
            if o["kind"] != _lib.OP_CONV:
                continue
            px = lambda i: t[i][0] * t[i][1] * t[i][2] * 2
            act = sum(px(i) for i in ins) + px(o["out"])
            wb = sum(o[k].numel() * 2 for k in ("weight", "weight2") if o.get(k) is not None)
            total += batch * act * (1 if det else T) + wb * (1 if det else chunks)
            launches += 1 if det else chunks
        return total, launches

    def close(self):
        if getattr(self, "handle", None) is not None and self.handle.value:
            self.lib.bmi_destroy(self.handle)
            self.handle = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class MCDEngine(CompiledGraph):
    """One model compiled for one GPU.  All methods are asynchronous on the current torch stream
    (the stream handle is what the C ABI receives); results are device tensors."""

    def __init__(self, model, device, max_batch=256, chunk_samples=None, dtype="f16"):
        device = torch.device(device)
        if device.type != "cuda":
            raise RuntimeError("MCDEngine needs a HIP device (torch device type 'cuda' on ROCm); there is no CPU path")
        if device.index is None:
            device = torch.device("cuda", torch.cuda.current_device())
        super().__init__(model, device, max_batch, chunk_samples, dtype)
        self.workspace = torch.empty(self.workspace_bytes, dtype=torch.uint8, device=device)
        # the non-finite counter of bmi_finalize_checked: allocated HERE, never lazily — a first finalize() inside a hipGraph capture
        # (BatchesInFlight.predict_graphed) would otherwise allocate it from the graph's private pool and re-zero it on every replay
        self._nonfinite = torch.zeros(1, dtype=torch.int32, device=device)
        # like the temperature (CompiledGraph.__init__), the ensemble weights and the vector or matrix scaling a model carries (EngineModelMixin's
        # set_exit_* setters, train/calibration.py) go to every engine built from it; their device copies live in one list, freed by close()
        self._cal_keep = []
        self.set_ensemble_weights(getattr(model, "exit_ensemble_weights", None))
        for attr, setter in (("exit_vector_scaling", self.set_vector_scaling), ("exit_matrix_scaling", self.set_matrix_scaling)):
            if getattr(model, attr, None) is not None:
                setter(*getattr(model, attr))

    ensemble_weights = None       # float64 [E, E] on the host, or None: the equal-weight mean (set_ensemble_weights)
    _map = CalibrationMap()       # the map in force (set_temperature / set_vector_scaling / set_matrix_scaling through _set_map); all ones is no temperature

    def close(self):
        self.__dict__.pop("_ens_scratch", None)      # (accumulate_ensemble's chunk of per-sample logits)
        super().close()                              # (the handle goes first: nothing reads the weight buffers any more)
        self.__dict__.pop("_cal_keep", None)

    def _set_map(self, kind, m):
        """What the three setters do with their resolved arguments ``m`` (``m.kind`` is ``kind``, or None: clear that kind — always allowed).
        A map goes in only while no OTHER kind is in force; then bmi_engine_set_<kind> gets the temperatures, or fresh device copies of the
        arrays.  A refused call leaves the engine as it was."""
        on = m.kind is not None and not (kind == "temperature" and all(t == 1.0 for t in m.tau))      # (all ones: off)
        if on and self._map.kind not in (None, kind):
            what, clear = _MAPS[self._map.kind][:2]
            raise ValueError(f"{_MAPS[kind][0]}: a {what} is set on this engine ({clear}(None) first: one calibration map at a time)")
        if kind == "temperature":
            super().set_temperature(m.tau)
        else:
            args = (None, None, 0, 0)
            if on:
                bufs = (torch.from_numpy(m.weight).to(self.device), torch.from_numpy(m.bias).to(self.device))
                self._cal_keep.append(bufs)          # never freed before close(): a captured launch may still hold an earlier pointer
                args = (C.c_void_p(bufs[0].data_ptr()), C.c_void_p(bufs[1].data_ptr()), self.n_exits, self.out_dim)
            _lib.check(getattr(self.lib, _MAPS[kind][2])(self.handle, *args), _MAPS[kind][2])
        if on:
            self._map = m
        elif self._map.kind == kind:
            self._map = CalibrationMap()

    def _resolve(self, who, **given):
        return resolve_calibration_map(**given, n_exits=self.n_exits, out_dim=self.out_dim, who=who)

    def _map_arrays(self, kind):
        return (self._map.weight, self._map.bias) if self._map.kind == kind else None

    def set_vector_scaling(self, scale, bias=None):
        """Per-class scale and bias of every exit's logits (bmi_engine_set_vector_scaling; Guo et al. 2017): ``scale`` / ``bias`` as
        ``check_vector_scaling`` takes them — [E, C], or [C] for every exit, ``bias`` None = zeros — or ``scale`` None: off.  From the next
        launch on every path through the fused head and the exit-ensemble launches computes softmax, mean, var, the entropies and the decisions
        of ``z_c = float32(float32(logit_c * scale[e][c]) + bias[e][c])``; ``logit_mean``, ``forward_once`` and ``forward_samples`` stay the raw
        logits, as under a temperature.  Off, the engine launches the kernels it did: the bits of an engine that never had one.  One map
        at a time: ValueError while a temperature (other than all ones) or a matrix scaling is set — clear it first.  The arrays live
        in device buffers the engine keeps; a hipGraph captured earlier keeps what it was captured with
        (``BatchesInFlight.set_vector_scaling`` discards them)."""
        self._set_map("vector", self._resolve("set_vector_scaling", scale=scale, bias=bias))

    @property
    def vector_scaling(self):
        """The vector scaling in force: (scale, bias), float32 [E, C] host arrays, or None when off."""
        return self._map_arrays("vector")

    def set_matrix_scaling(self, matrix, bias=None):
        """A full [C, C] matrix and a bias on every exit's logits (bmi_engine_set_matrix_scaling; Guo et al. 2017): ``matrix`` / ``bias`` as
        ``check_matrix_scaling`` takes them — [E, C, C] or [C, C] for every exit, row = output class; ``bias`` [E, C], [C] or None = zeros — or
        ``matrix`` None: off.  From the next launch on every path through the fused head and the exit-ensemble launches computes softmax,
        mean, var, the entropies and the decisions of ``z = M l + b`` in the head's fp32 — per class the products in ascending j, each
        rounded, added one by one, the bias last (``train.calibration.matrix_logits`` restates it exactly; a diagonal matrix gives
        ``set_vector_scaling``'s bits).  ``logit_mean``, ``forward_once`` and ``forward_samples`` stay the raw logits.  Off, the engine launches
        the kernels it did.  One map at a time: ValueError while a temperature (other than all ones) or a vector scaling is set.
        The arrays live in device buffers the engine keeps until ``close()``; a hipGraph captured earlier keeps what it was captured with
        (``BatchesInFlight.set_matrix_scaling`` discards them)."""
        self._set_map("matrix", self._resolve("set_matrix_scaling", matrix=matrix, bias=bias))

    @property
    def matrix_scaling(self):
        """The matrix scaling in force: (matrix [E, C, C], bias [E, C]), float32 host arrays, or None when off."""
        return self._map_arrays("matrix")

    def set_temperature(self, tau):
        self._set_map("temperature", self._resolve("set_temperature", tau=tau))
    set_temperature.__doc__ = CompiledGraph.set_temperature.__doc__

    def set_ensemble_weights(self, w):
        """The weights of the exit ensembles (bmi_engine_set_ensemble_weights): ``w`` as ``check_ensemble_weights`` takes it — None (off),
        an [E] vector or an [E, E] matrix.  From the next launch on every consumer of the ensemble is the WEIGHTED one's, q_te = sum_{i<=e}
        W[e][i] p_ti per sample in exit order: ``predict_ensemble`` / ``accumulate_ensemble``, ``predict_adaptive(ensemble=True)`` with its
        ``stop_on="ensemble"`` rule, ``predict_early_exit``'s ``ensemble=True`` rule, ``ensemble_readout`` and ``best_preds``.  mean, var and
        the per-exit entropies never depend on it; ``predict_with_exit`` (the older entry) has no ensemble rule.  Off, the engine launches the
        unweighted kernels: the bits of an engine that never had weights.  The matrix lives in a small device buffer the engine keeps; a
        hipGraph captured earlier keeps the weights it was captured with (``model.set_exit_ensemble_weights`` drops the pipes that hold such graphs)."""
        W = check_ensemble_weights(w, self.n_exits)
        self._ens_w_dev = None                       # (what exit_stat_records hands to bmi_exit_stat_record)
        if W is None:
            rc = self.lib.bmi_engine_set_ensemble_weights(self.handle, None, 0)
        else:
            buf = self._ens_w_dev = torch.from_numpy(W).to(self.device)
            self._cal_keep.append(buf)               # never freed before close(): a captured launch may still hold an earlier pointer
            rc = self.lib.bmi_engine_set_ensemble_weights(self.handle, C.c_void_p(buf.data_ptr()), self.n_exits)
        _lib.check(rc, "bmi_engine_set_ensemble_weights")
        self.ensemble_weights = W

    # ---- the path ------------------------------------------------------------------------------
    def _stream(self):
        return C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)

    def _check_x(self, x):
        if not (isinstance(x, torch.Tensor) and x.is_cuda and x.device == self.device):
            raise RuntimeError(f"input must live on {self.device}")
        if x.dtype != torch.float32 or x.dim() != 4 or tuple(x.shape[1:]) != (3, 32, 32):
            raise ValueError(f"expected float32 [B,3,32,32] like the reference's loaders, got {x.dtype} {tuple(x.shape)}")
        if x.shape[0] > self.max_batch:
            raise ValueError(f"batch {x.shape[0]} exceeds the engine's max_batch {self.max_batch}")
        return x.contiguous()

    def new_moments(self, batch):
        """Zeroed float64 accumulators S1 = sum p, S2 = sum p^2, SL = sum logit, each [E, B, C]."""
        return torch.zeros(3, self.n_exits, batch, self.out_dim, dtype=torch.float64, device=self.device)

    def accumulate(self, x, S, t_begin, t_count, seed=0, cnt0=0, image_offset=0):
        """Adds samples t_begin .. t_begin+t_count-1 of batch ``x`` into the moment buffer ``S``.
        ``image_offset``: ``x`` (and ``S``) are images image_offset.. of a larger batch — the masks are drawn at the images'
        indices in the whole batch (bmi_forward_mcd_images: one rank's share of a batch partitioned by images)."""
        self._forward(x, S, None, t_begin, t_count, seed, cnt0, image_offset)
        return S

    def _check_sums(self, B, S, H, Q=None, QH=None, ensemble=False):
        """The float64 sums of a batch of B images a forward call adds into: S [3, E, B, C] (``new_moments``) and, where given, H [E, B]
        (``new_uncertainty_sums``), Q [2, E, B, C] and QH [E, B] (``new_ensemble_sums``); ``ensemble``: the call needs all four."""
        E, Cd = self.n_exits, self.out_dim
        for buf, shape, name, needed in ((S, (3, E, B, Cd), "moment buffer S", True), (H, (E, B), "entropy buffer H", ensemble),
                                         (Q, (2, E, B, Cd), "ensemble buffer Q", ensemble), (QH, (E, B), "ensemble entropy buffer QH", ensemble)):
            if needed or buf is not None:
                check_buffer(buf, shape, torch.float64, self.device, name)

    def _scratch(self, name, need):
        """The engine's byte buffer ``name`` on the device, grown on demand to ``need`` bytes (never shrunk)."""
        buf = self.__dict__.get(name)
        if buf is None or buf.numel() < need:
            buf = self.__dict__[name] = torch.empty(need, dtype=torch.uint8, device=self.device)
        return buf

    def _forward(self, x, S, H, t_begin, t_count, seed, cnt0, image_offset):
        """``accumulate`` (H None: bmi_forward_mcd_images) and ``accumulate_uncertainty`` (bmi_forward_mcd_entropy)."""
        x = self._check_x(x)
        B = x.shape[0]
        self._check_sums(B, S, H)
        name = "bmi_forward_mcd_images" if H is None else "bmi_forward_mcd_entropy"
        with torch.cuda.device(self.device):
            rc = getattr(self.lib, name)(self.handle, x.data_ptr(), B, int(image_offset), int(t_begin), int(t_count),
                                         int(seed) & 0xFFFFFFFFFFFFFFFF, int(cnt0), S[0].data_ptr(), S[1].data_ptr(), S[2].data_ptr(),
                                         *(() if H is None else (H.data_ptr(),)), self.workspace.data_ptr(), self.workspace_bytes, self._stream())
        _lib.check(rc, name)

    def image_offset_ok(self, image_offset):
        """Whether a share of a batch that starts at image ``image_offset`` can be run by ``accumulate(..., image_offset=)``
        (bmi_image_offset_ok: host-only, every site's index offset must be a whole number of Philox calls)."""
        rc = self.lib.bmi_image_offset_ok(self.handle, int(image_offset))
        if rc not in (_lib.BMI_OK, -95):
            _lib.check(rc, "bmi_image_offset_ok")
        return rc == _lib.BMI_OK

    def finalize(self, S, t_total):
        """mean / var (ddof=0) / mean logit, float64 [E, B, C] each.  Also counts the non-finite sums into the engine's device counter
        (bmi_finalize_checked; no synchronisation here): ``check_finite()`` reads it when the results are read."""
        out = torch.empty_like(S)
        n = S[0].numel()
        with torch.cuda.device(self.device):
            rc = self.lib.bmi_finalize_checked(n, int(t_total), S[0].data_ptr(), S[1].data_ptr(), S[2].data_ptr(),
                                               out[0].data_ptr(), out[1].data_ptr(), out[2].data_ptr(), self._nonfinite.data_ptr(), self._stream())
        _lib.check(rc, "bmi_finalize_checked")
        return dict(mean=out[0], var=out[1], logit_mean=out[2])

    _nonfinite = None

    def nonfinite_count(self, reset=True):
        """Elements of the moment buffers finalized since the last reset whose sums were inf / NaN (a host read: synchronises)."""
        if self._nonfinite is None:
            return 0
        n = int(self._nonfinite.item())
        if reset and n:
            self._nonfinite.zero_()
        return n

    def check_finite(self):
        """Raises FloatingPointError if a finalize since the last check saw non-finite sums — on the 16-bit engines an activation past
        65 504 (fp16) turns into inf and then NaN in the softmax; the reference's fp32 path would have carried the value.  Callers that pull
        results to the host (FullAnalysis, evaluate, bench) call this right there."""
        n = self.nonfinite_count()
        if n:
            raise FloatingPointError(f"{n} non-finite moment sums on the {self.dtype!r} engine (overflow of a 16-bit activation?): "
                                     "use engine_dtype='f16x2' / 'bf16x3' (or 'auto', which checks this on the first batch)")

    def set_option(self, name, value):
        """A kernel-selection switch of THIS engine (bmi_engine_set_option): the engine was created with a copy of the process defaults
        (``_lib.set_option``) and keeps it whatever those become."""
        _lib.check(self.lib.bmi_engine_set_option(self.handle, name.encode(), int(value)), f"bmi_engine_set_option({name})")

    def predict(self, x, T, seed=0, t_begin=0, cnt0=0):
        S = self.new_moments(x.shape[0])
        self.accumulate(x, S, t_begin, T, seed, cnt0)
        return self.finalize(S, T)

    # ---- uncertainty decomposition (bmi_forward_mcd_entropy / bmi_finalize_uncertainty) ------------------------------------------
    def new_uncertainty_sums(self, batch):
        """Zeroed float64 accumulators of ``accumulate_uncertainty``: S [3, E, B, C] (``new_moments``' S1 / S2 / SL) and H [E, B] (the sums
        of the per-sample entropies), views of ONE allocation (``S._base``) so that a sharded caller all-reduces both in one call."""
        from .sharding import new_uncertainty_sums
        return new_uncertainty_sums(self.n_exits, batch, self.out_dim, self.device)

    def accumulate_uncertainty(self, x, S, H, t_begin, t_count, seed=0, cnt0=0, image_offset=0):
        """``accumulate`` (the same bits in S) that also adds every sample's softmax entropy into H [E, B]: computed in the fused head where
        the per-sample softmax exists, so nothing per-sample reaches memory (``forward_samples`` would write [T, E, B, C] logits)."""
        self._forward(x, S, H, t_begin, t_count, seed, cnt0, image_offset)
        return S, H

    def finalize_uncertainty(self, S, H, t_total):
        """``finalize``'s dict plus, float64 [E, B] each: ``pred_entropy`` H[mean] (total uncertainty), ``exp_entropy`` E_t H[p_t]
        (aleatoric) and ``mutual_info`` their difference clamped at 0 (epistemic, "BALD").  Non-finite inputs count into the engine's
        counter like finalize's (``check_finite``)."""
        r = self.finalize(S, t_total)
        E, B, Cd = S.shape[1], S.shape[2], S.shape[3]
        check_buffer(H, (E, B), torch.float64, self.device, "entropy buffer H")
        out = torch.empty(3, E, B, dtype=torch.float64, device=S.device)
        with torch.cuda.device(self.device):
            rc = self.lib.bmi_finalize_uncertainty(E, B, Cd, int(t_total), S[0].data_ptr(), H.data_ptr(), out[0].data_ptr(), out[1].data_ptr(),
                                                   out[2].data_ptr(), self._nonfinite.data_ptr(), self._stream())
        _lib.check(rc, "bmi_finalize_uncertainty")
        r.update(pred_entropy=out[0], exp_entropy=out[1], mutual_info=out[2])
        return r

    def predict_uncertainty(self, x, T, seed=0, t_begin=0, cnt0=0):
        """``predict`` plus the uncertainty decomposition of ``finalize_uncertainty``."""
        S, H = self.new_uncertainty_sums(x.shape[0])
        self.accumulate_uncertainty(x, S, H, t_begin, T, seed, cnt0)
        return self.finalize_uncertainty(S, H, T)

    # ---- the exit ensemble as a predictor (bmi_forward_mcd_ensemble / bmi_finalize_ensemble / bmi_ensemble_moments) -----------------
    def new_ensemble_sums(self, batch):
        """Zeroed float64 accumulators of ``accumulate_ensemble``: S [3, E, B, C] and H [E, B] (``new_uncertainty_sums``), Q [2, E, B, C]
        (the sums of the per-sample exit ensembles q and of q^2) and QH [E, B] (the sums of their entropies) — views of ONE allocation
        (``S._base``), so that a sharded caller all-reduces all four in one call: every one of them is additive over samples."""
        E, Cd = self.n_exits, self.out_dim
        ns, nh, nq = 3 * E * batch * Cd, E * batch, 2 * E * batch * Cd
        buf = torch.zeros(ns + nh + nq + nh, dtype=torch.float64, device=self.device)
        return (buf[:ns].view(3, E, batch, Cd), buf[ns:ns + nh].view(E, batch), buf[ns + nh:ns + nh + nq].view(2, E, batch, Cd),
                buf[ns + nh + nq:].view(E, batch))

    def _ensemble_scratch(self):
        """One chunk of per-sample logits (bmi_ensemble_scratch_bytes), allocated once per engine — for ``max_batch`` — on first use."""
        if "_ens_scratch" not in self.__dict__:
            self._scratch("_ens_scratch", max(int(self.lib.bmi_ensemble_scratch_bytes(self.handle, self.max_batch)), 1))
        return self.__dict__["_ens_scratch"]

    def accumulate_ensemble(self, x, S, H, Q, QH, t_begin, t_count, seed=0, cnt0=0, image_offset=0):
        """``accumulate_uncertainty`` (the same bits in S and H) that also adds, per sample, the exit ensembles q_e = mean of the softmax
        outputs of exits 0..e of THAT sample into Q[0], their squares into Q[1] and their entropies into QH: the heads of a chunk leave
        their logits in the engine's scratch and one kernel behind them (csrc/ensemble.hip) adds the chunk in sample order onto the
        running sums — the same bits however the samples are split into calls.  The members are the tempered distributions when a
        temperature is set (``set_temperature``)."""
        x = self._check_x(x)
        B = x.shape[0]
        self._check_sums(B, S, H, Q, QH, ensemble=True)
        scratch = self._ensemble_scratch()
        with torch.cuda.device(self.device):
            rc = self.lib.bmi_forward_mcd_ensemble(self.handle, x.data_ptr(), B, int(image_offset), int(t_begin), int(t_count),
                                                   int(seed) & 0xFFFFFFFFFFFFFFFF, int(cnt0), S[0].data_ptr(), S[1].data_ptr(), S[2].data_ptr(),
                                                   H.data_ptr(), Q[0].data_ptr(), Q[1].data_ptr(), QH.data_ptr(), scratch.data_ptr(),
                                                   scratch.numel(), self.workspace.data_ptr(), self.workspace_bytes, self._stream())
        _lib.check(rc, "bmi_forward_mcd_ensemble")
        return S, H, Q, QH

    def _finalize_ensemble_sums(self, Q, QH, t_total, t_used=None):
        """The five ``ens_*`` entries of ``finalize_ensemble`` from the sums Q [2, E, B, C] and QH [E, B]: divided by ``t_total``
        (bmi_finalize_ensemble), or image b's by t_used[b] when ``t_used`` is given (bmi_finalize_ensemble_per_image)."""
        check_buffer(Q, (2, None, None, None), torch.float64, self.device, "ensemble buffer Q")
        _, E, B, Cd = Q.shape
        check_buffer(QH, (E, B), torch.float64, self.device, "ensemble entropy buffer QH")
        if t_used is not None:
            check_buffer(t_used, (B,), torch.int32, self.device, "t_used")
        name = "bmi_finalize_ensemble" if t_used is None else "bmi_finalize_ensemble_per_image"
        count = int(t_total) if t_used is None else t_used.data_ptr()
        mv = torch.empty(2, E, B, Cd, dtype=torch.float64, device=self.device)
        ent = torch.empty(3, E, B, dtype=torch.float64, device=self.device)
        with torch.cuda.device(self.device):
            rc = getattr(self.lib, name)(E, B, Cd, count, Q[0].data_ptr(), Q[1].data_ptr(), QH.data_ptr(), mv[0].data_ptr(), mv[1].data_ptr(),
                                         ent[0].data_ptr(), ent[1].data_ptr(), ent[2].data_ptr(), self._nonfinite.data_ptr(), self._stream())
        _lib.check(rc, name)
        return dict(ens_mean=mv[0], ens_var=mv[1], ens_pred_entropy=ent[0], ens_exp_entropy=ent[1], ens_mutual_info=ent[2])

    def finalize_ensemble_per_image(self, Q, QH, t_used):
        """The five ``ens_*`` entries of ``finalize_ensemble`` with image b's sums divided by its own sample count t_used[b]
        (bmi_finalize_ensemble_per_image; device int32 [B], every entry >= 1): the read-out of ``accumulate_adaptive(ensemble=True)``."""
        return self._finalize_ensemble_sums(Q, QH, None, t_used)

    def finalize_ensemble(self, S, H, Q, QH, t_total):
        """``finalize_uncertainty``'s dict plus the read-out of the exit ensembles, float64: ``ens_mean`` and ``ens_var`` (ddof 0) [E, B, C],
        ``ens_pred_entropy`` H[ens_mean], ``ens_exp_entropy`` E_t H[q_t] and ``ens_mutual_info`` (clamped at 0) [E, B]; row 0 is exit 0
        itself.  Non-finite sums count into the engine's counter (``check_finite``)."""
        r = self.finalize_uncertainty(S, H, t_total)
        r.update(self._finalize_ensemble_sums(Q, QH, t_total))
        return r

    def predict_ensemble(self, x, T, seed=0, t_begin=0, cnt0=0):
        """``predict_uncertainty`` plus the five ``ens_*`` entries of ``finalize_ensemble``."""
        S, H, Q, QH = self.new_ensemble_sums(x.shape[0])
        self.accumulate_ensemble(x, S, H, Q, QH, t_begin, T, seed, cnt0)
        return self.finalize_ensemble(S, H, Q, QH, T)

    def _held_logits_map(self, who, logits, tau, weights, scale, bias, matrix):
        """What ``ensemble_moments`` and ``vote_counts`` start from: the shape (T, E, B, C) of the checked ``logits``, the kind of the one map
        among ``tau`` / ``scale`` / ``matrix`` (``resolve_calibration_map``), and the C arguments — the temperatures as a float array, the
        map's two arrays and the checked ensemble weights as device tensors (``_ptr`` below) — each None where not given.  The caller holds the
        device copies until its launch is queued; they are then freed in stream order behind it."""
        shape = check_buffer(logits, (None,) * 4, torch.float32, self.device, "logits [T, E, B, C]").shape
        m = resolve_calibration_map(tau, scale, bias, matrix, n_exits=shape[1], out_dim=shape[3], who=who)
        W = check_ensemble_weights(weights, shape[1])
        tau_c = None if m.tau is None else (C.c_float * shape[1])(*m.tau)
        with torch.cuda.device(self.device):
            dev = [None if h is None else torch.from_numpy(h).to(self.device) for h in (m.weight, m.bias, W)]
        return (shape, m.kind, tau_c, *dev)

    def ensemble_moments(self, logits, tau=None, out=None, t_before=0, weights=None, scale=None, bias=None, matrix=None):
        """The exit-ensemble read-out of per-sample logits the caller holds (bmi_ensemble_moments + bmi_finalize_ensemble): ``logits`` fp32
        [T, E, B, C] on the engine's device (``forward_samples``), ``tau`` None, a scalar or E temperatures (independent of the one set on
        this engine).  Returns the five ``ens_*`` entries of ``finalize_ensemble`` plus the sums ``Q`` [2, E, B, C] and ``QH`` [E, B];
        ``out=(Q, QH)`` ADDS into the sums of earlier calls that held ``t_before`` samples — the same bits as one call on all of them —
        and the results describe all ``t_before + T``.  ``weights`` (``check_ensemble_weights``: None, [E] or [E, E]; independent of the ones
        set on this engine): the weighted ensembles, bmi_ensemble_moments_weighted.  ``scale`` / ``bias`` (``check_vector_scaling``; not together
        with ``tau``): the members under a vector scaling, bmi_ensemble_moments_vector, with or without ``weights``.  ``matrix`` / ``bias``
        (``check_matrix_scaling``; not together with ``tau`` or ``scale``): the members under a matrix scaling, bmi_ensemble_moments_matrix.
        ``train.uncertainty.decompose_ensemble_logits`` is the host restatement."""
        (T, E, B, Cd), kind, tau_c, a, b, w = self._held_logits_map("ensemble_moments", logits, tau, weights, scale, bias, matrix)
        if out is None:
            Q = torch.zeros(2, E, B, Cd, dtype=torch.float64, device=self.device)
            QH = torch.zeros(E, B, dtype=torch.float64, device=self.device)
        else:
            Q, QH = out
            check_buffer(Q, (2, E, B, Cd), torch.float64, self.device, "out[0] (Q)")
            check_buffer(QH, (E, B), torch.float64, self.device, "out[1] (QH)")
        if kind in ("vector", "matrix"):
            name, cal = f"bmi_ensemble_moments_{kind}", (_ptr(a), _ptr(b), _ptr(w))
        elif w is not None:
            name, cal = "bmi_ensemble_moments_weighted", (tau_c, _ptr(w))
        else:
            name, cal = "bmi_ensemble_moments", (tau_c,)
        with torch.cuda.device(self.device):
            rc = getattr(self.lib, name)(logits.data_ptr(), T, E, B, Cd, *cal, Q[0].data_ptr(), Q[1].data_ptr(), QH.data_ptr(), self._stream())
        _lib.check(rc, name)
        r = self._finalize_ensemble_sums(Q, QH, int(t_before) + T)
        r.update(Q=Q, QH=QH)
        return r

    # ---- vote counts: variation ratio and majority vote (bmi_forward_mcd_votes / bmi_vote_counts / bmi_finalize_votes) ----------------
    def new_vote_counts(self, batch):
        """Zeroed int32 vote counts V [2, E, B, C] of ``accumulate_votes``: V[0] the exits' votes, V[1] the exit ensembles'.  Integers:
        additive over samples, chunks, calls and ranks."""
        return torch.zeros(2, self.n_exits, batch, self.out_dim, dtype=torch.int32, device=self.device)

    def accumulate_votes(self, x, S, H, Q, QH, V, t_begin, t_count, seed=0, cnt0=0, image_offset=0):
        """``accumulate_ensemble`` (the same bits in S, H, Q and QH) that also adds every pass's votes into V [2, E, B, C] (``new_vote_counts``):
        V[0, e, b, k] += 1 for k the arg-max of exit e's calibrated logits of that pass, V[1, e, b, k] += 1 for k the arg-max of the exit
        ensemble q_e of that pass (the weighted one under ``set_ensemble_weights``), the lowest class index on ties.  One kernel
        (csrc/votes.hip) behind every chunk's ensemble launch reads the same per-sample logits; a (pass, exit, image) row with a non-finite
        calibrated logit casts no vote, nor do the ensembles behind it, and counts into the engine's counter (``check_finite``)."""
        x = self._check_x(x)
        B = x.shape[0]
        self._check_sums(B, S, H, Q, QH, ensemble=True)
        check_buffer(V, (2, self.n_exits, B, self.out_dim), torch.int32, self.device, "vote counts V")
        scratch = self._ensemble_scratch()
        with torch.cuda.device(self.device):
            rc = self.lib.bmi_forward_mcd_votes(self.handle, x.data_ptr(), B, int(image_offset), int(t_begin), int(t_count),
                                                int(seed) & 0xFFFFFFFFFFFFFFFF, int(cnt0), S[0].data_ptr(), S[1].data_ptr(), S[2].data_ptr(),
                                                H.data_ptr(), Q[0].data_ptr(), Q[1].data_ptr(), QH.data_ptr(), V.data_ptr(),
                                                self._nonfinite.data_ptr(), scratch.data_ptr(), scratch.numel(), self.workspace.data_ptr(),
                                                self.workspace_bytes, self._stream())
        _lib.check(rc, "bmi_forward_mcd_votes")
        return S, H, Q, QH, V

    def finalize_votes(self, V):
        """The read-out of vote counts V [2, E, B, C] (bmi_finalize_votes), device tensors: ``votes`` int32 [E, B, C] (V[0] itself),
        ``vote_class`` int32 [E, B] the majority vote (the lowest class with the modal count; -1 where no vote was cast),
        ``variation_ratio`` float64 [E, B] = 1 - modal count / votes cast (1.0 where none), ``vote_entropy`` float64 [E, B] the entropy of
        the vote shares in nats (0.0 where none) — and their ``ens_*`` twins for the exit ensembles (V[1]).
        ``train.uncertainty.vote_readout_numpy`` is the host restatement."""
        check_buffer(V, (2, None, None, None), torch.int32, self.device, "vote counts V")
        _, E, B, Cd = V.shape
        cls = torch.empty(2, E, B, dtype=torch.int32, device=self.device)
        out = torch.empty(2, 2, E, B, dtype=torch.float64, device=self.device)
        with torch.cuda.device(self.device):
            rc = self.lib.bmi_finalize_votes(E, B, Cd, V.data_ptr(), cls.data_ptr(), out[0].data_ptr(), out[1].data_ptr(), self._stream())
        _lib.check(rc, "bmi_finalize_votes")
        return dict(votes=V[0], vote_class=cls[0], variation_ratio=out[0, 0], vote_entropy=out[1, 0],
                    ens_votes=V[1], ens_vote_class=cls[1], ens_variation_ratio=out[0, 1], ens_vote_entropy=out[1, 1])

    def predict_votes(self, x, T, seed=0, t_begin=0, cnt0=0):
        """``predict_ensemble``'s dict plus the eight entries of ``finalize_votes``."""
        S, H, Q, QH = self.new_ensemble_sums(x.shape[0])
        V = self.new_vote_counts(x.shape[0])
        self.accumulate_votes(x, S, H, Q, QH, V, t_begin, T, seed, cnt0)
        r = self.finalize_ensemble(S, H, Q, QH, T)
        r.update(self.finalize_votes(V))
        return r

    def vote_counts(self, logits, tau=None, weights=None, scale=None, bias=None, matrix=None, out=None, rows=None, n_exits_of_image=None):
        """The vote counts of per-sample logits the caller holds (bmi_vote_counts): ``logits`` fp32 [T, E, B, C] on the engine's device
        (``forward_samples``); ``tau``, ``weights``, ``scale`` / ``bias`` and ``matrix`` / ``bias`` as ``ensemble_moments`` takes them (at
        most one map; all independent of what is set on this engine).  Returns V int32 [2, E, B, C]; ``out=V`` ADDS into the counts of
        earlier calls.  ``train.uncertainty.vote_counts_numpy`` is the host restatement; ``finalize_votes`` reads V out.
        ``rows`` (int32 [n], 1 <= n <= B, image indices, each at most once) and ``n_exits_of_image`` (int32 [B]), device tensors or
        anything ``torch.as_tensor`` takes: the image-list form (bmi_vote_counts_rows) — only the listed images, and of image b only its
        first ``n_exits_of_image[b]`` exits, are read and counted; everything else in V is left as it is."""
        (T, E, B, Cd), kind, tau_c, a, b, w = self._held_logits_map("vote_counts", logits, tau, weights, scale, bias, matrix)
        if out is None:
            V = torch.zeros(2, E, B, Cd, dtype=torch.int32, device=self.device)
        else:
            V = check_buffer(out, (2, E, B, Cd), torch.int32, self.device, "out (V)")
        vec, mat = (None, _ptr(a)) if kind == "matrix" else (_ptr(a), None)
        if rows is not None or n_exits_of_image is not None:
            lst = ne = None
            if rows is not None:
                lst = torch.as_tensor(rows, dtype=torch.int32, device=self.device).contiguous()
                if lst.dim() != 1 or not 1 <= lst.numel() <= B:
                    raise ValueError(f"rows must be a 1-d list of 1 .. {B} image indices, got shape {tuple(lst.shape)}")
            if n_exits_of_image is not None:
                ne = torch.as_tensor(n_exits_of_image, dtype=torch.int32, device=self.device).contiguous()
                if tuple(ne.shape) != (B,):
                    raise ValueError(f"n_exits_of_image must have shape ({B},), got {tuple(ne.shape)}")
            with torch.cuda.device(self.device):
                rc = self.lib.bmi_vote_counts_rows(logits.data_ptr(), T, E, B, Cd, tau_c, vec, _ptr(b), mat, _ptr(w), _ptr(lst),
                                                   0 if lst is None else lst.numel(), _ptr(ne), V.data_ptr(), self._nonfinite.data_ptr(),
                                                   self._stream())
            _lib.check(rc, "bmi_vote_counts_rows")
            return V
        with torch.cuda.device(self.device):
            rc = self.lib.bmi_vote_counts(logits.data_ptr(), T, E, B, Cd, tau_c, vec, _ptr(b), mat, _ptr(w), V.data_ptr(),
                                          self._nonfinite.data_ptr(), self._stream())
        _lib.check(rc, "bmi_vote_counts")
        return V

    def vote_decide(self, V, t, T_max, slack=0, kind=0, test_exit=-1, active=None):
        """The decided-vote stop rule on counts the caller holds (bmi_vote_decide; ``rule="votes"`` of ``accumulate_adaptive``): V int32
        [2, E, B, C] after ``t`` of ``T_max`` passes, row ``V[kind, test_exit]`` (kind 0: the exit, 1: the exit ensemble), over the images
        ``active`` (int32 list, default all).  Returns (still_active int32 [n] in order, t_used int32 [B]: ``t`` for every tested image,
        -1 elsewhere).  ``train.uncertainty.vote_decided_numpy`` is the host restatement."""
        check_buffer(V, (2, None, None, None), torch.int32, self.device, "vote counts V")
        _, E, B, Cd = V.shape
        test_exit = int(test_exit) + (E if int(test_exit) < 0 else 0)
        lst = None if active is None else torch.as_tensor(active, dtype=torch.int32, device=self.device).contiguous()
        n = B if lst is None else lst.numel()
        out = torch.empty(max(n, 1), dtype=torch.int32, device=self.device)
        count = torch.zeros(1, dtype=torch.int32, device=self.device)
        t_used = torch.full((B,), -1, dtype=torch.int32, device=self.device)
        with torch.cuda.device(self.device):
            rc = self.lib.bmi_vote_decide(V.data_ptr(), E, B, Cd, int(kind), test_exit, int(t), int(T_max), int(slack), _ptr(lst), n,
                                          out.data_ptr(), count.data_ptr(), t_used.data_ptr(), self._stream())
        _lib.check(rc, "bmi_vote_decide")
        return out[:int(count.item())], t_used

    def predict_with_exit(self, x, T, threshold, seed=0, cnt0=0, first_exit=1):
        """Confidence-threshold early exiting on the device (bmi_forward_mcd_exit): an image leaves after the first exit
        e >= ``first_exit`` whose T-mean confidence exceeds ``threshold`` (the reference's ``confidence_exiting`` rule,
        SA/train/results_analyzer.py:606-630; its loop starts at exit 1) and the later stages only run for the images
        that are still active.  Returns dict(mean/var/logit_mean [E,B,C] — rows of exits an image never reached are
        meaningless —, exit_layer int32 [B], active_after [E] (host ints), best_preds [B,C] = mean[exit_layer[b], b])."""
        x = self._check_x(x)
        B = x.shape[0]
        if T > self.chunk_samples:
            raise ValueError(f"dynamic exiting needs all T={T} samples in one chunk (engine planned for {self.chunk_samples})")
        S = self.new_moments(B)
        exit_layer = torch.empty(B, dtype=torch.int32, device=self.device)
        active = (C.c_int32 * self.n_exits)()
        with torch.cuda.device(self.device):
            rc = self.lib.bmi_forward_mcd_exit(self.handle, x.data_ptr(), B, int(T), int(seed) & 0xFFFFFFFFFFFFFFFF, int(cnt0),
                                               float(threshold), int(first_exit), S[0].data_ptr(), S[1].data_ptr(), S[2].data_ptr(),
                                               exit_layer.data_ptr(), active, self.workspace.data_ptr(), self.workspace_bytes,
                                               self._stream())
        _lib.check(rc, "bmi_forward_mcd_exit")
        r = self.finalize(S, T)
        r["exit_layer"] = exit_layer
        r["active_after"] = [int(v) for v in active]
        r["best_preds"] = r["mean"][exit_layer.long(), torch.arange(B, device=self.device)]
        return r

    def accumulate_early_exit(self, x, S, T, threshold, seed=0, cnt0=0, first_exit=1, rule="confidence", ensemble=False, H=None, Q=None,
                              QH=None, V=None):
        """The sampling half of ``predict_early_exit`` (bmi_forward_mcd_exit_staged) into the ZEROED sums S [3, E, B, C] (and H [E, B]:
        ``new_uncertainty_sums``): every row it computes equals ``accumulate``'s over samples 0 .. T-1 bit for bit, rows of exits an image
        never reached stay zero.  With ``Q`` and ``QH`` (and H; all ZEROED: ``new_ensemble_sums``) the exit-ensemble sums of the exits every
        image reached as well (bmi_forward_mcd_exit_staged_ensemble): rows e <= exit_layer[b] are ``accumulate_ensemble``'s bits, the others
        stay zero; the rule is not changed.  With ``V`` (ZEROED: ``new_vote_counts``; needs Q / QH / H) the vote counts of the exits every
        image reached as well (bmi_forward_mcd_exit_staged_votes): rows e <= exit_layer[b] of V[0] and V[1] are ``accumulate_votes``' counts,
        the others stay zero.  Returns (exit_layer int32 [B] on the device, active_after host list [E])."""
        x = self._check_x(x)
        B = x.shape[0]
        if rule not in _lib.EXIT_RULES:
            raise ValueError(f"rule must be one of {sorted(_lib.EXIT_RULES)}, got {rule!r}")
        T, first_exit = int(T), int(first_exit)
        if not 1 <= T <= self.chunk_samples:
            raise ValueError(f"early exiting needs all T={T} samples in one chunk (engine planned for {self.chunk_samples})")
        if not 0 <= first_exit < self.n_exits:
            raise ValueError(f"first_exit must be in [0, {self.n_exits})")
        if (Q is None) != (QH is None):
            raise ValueError("the ensemble read-out needs both Q and QH (new_ensemble_sums)")
        if V is not None and (Q is None or H is None):
            raise ValueError("the vote counts V need the ensemble sums Q / QH and H (new_ensemble_sums)")
        self._check_sums(B, S, H, Q, QH, ensemble=Q is not None)
        if V is not None:
            check_buffer(V, (2, self.n_exits, B, self.out_dim), torch.int32, self.device, "vote counts V")
        exit_layer = torch.empty(B, dtype=torch.int32, device=self.device)
        active = (C.c_int32 * self.n_exits)()
        r_c = _lib.ExitRule(_lib.EXIT_RULES[rule], int(bool(ensemble)), float(threshold), first_exit)
        name = "bmi_forward_mcd_exit_staged" if Q is None else "bmi_forward_mcd_exit_staged_ensemble" if V is None else "bmi_forward_mcd_exit_staged_votes"
        scratch = None if Q is None else self._ensemble_scratch()
        votes = () if V is None else (V.data_ptr(), self._nonfinite.data_ptr())
        ens = () if Q is None else (Q[0].data_ptr(), Q[1].data_ptr(), QH.data_ptr(), *votes, scratch.data_ptr(), scratch.numel())
        with torch.cuda.device(self.device):
            rc = getattr(self.lib, name)(self.handle, x.data_ptr(), B, T, int(seed) & 0xFFFFFFFFFFFFFFFF, int(cnt0), C.byref(r_c), S[0].data_ptr(),
                                         S[1].data_ptr(), S[2].data_ptr(), None if H is None else H.data_ptr(), *ens, exit_layer.data_ptr(), active,
                                         self.workspace.data_ptr(), self.workspace_bytes, self._stream())
        _lib.check(rc, name)
        return exit_layer, [int(v) for v in active]

    def predict_early_exit(self, x, T, threshold, seed=0, cnt0=0, first_exit=1, rule="confidence", ensemble=False, uncertainty=False,
                           ensemble_readout=False, votes=False):
        """Early exiting by stages on the device (bmi_forward_mcd_exit_staged): unlike ``predict_with_exit`` the later stages skip the
        deterministic trunk too, so with exit-only dropout an image that leaves at exit 1 never runs layer3 / layer4.  After exit e >=
        ``first_exit`` an image leaves when its statistic exceeds ``threshold``: ``rule="confidence"`` max_c p_c (the reference's
        is_confident), ``"margin"`` top-1 minus top-2 (confident(diff=True)); p = the T-mean softmax of exit e, or with ``ensemble`` the mean
        of exits 0..e (the reference's exit ensembles).  Every computed row equals ``predict``'s bit for bit.  Returns
        ``predict_with_exit``'s dict (``best_preds``: the ensemble mean at the exit taken when ``ensemble``), plus ``macs_done`` (MACs the
        stages ran: per stage, images that ran it x (prefix MACs + T x suffix MACs), ops without a row-table form at the whole batch) and
        ``macs_full`` (``predict``'s); with ``uncertainty``, also pred_entropy / exp_entropy / mutual_info [E,B] of the computed rows as in
        ``finalize_uncertainty``.  With ``ensemble_readout`` (``ensemble`` keeps its meaning: it selects the rule), also the entropies
        above and the five ``ens_*`` entries of ``finalize_ensemble`` over ``T`` — the per-sample exit ensembles, from one kernel launch
        behind the last stage that ran; rows of exits an image never reached are meaningless — and ``best_ens``: dict(mean, var [B, C],
        pred_entropy, exp_entropy, mutual_info [B]) of the ensemble of exits 0..exit_layer[b].  With ``votes`` (needs
        ``ensemble_readout``) also the eight entries of ``finalize_votes`` and ``V``: rows e <= exit_layer[b] are ``predict_votes``', the
        rows of exits an image never reached hold no votes (vote_class -1).  Synchronises once per decision."""
        if votes and not ensemble_readout:
            raise ValueError("votes=True needs ensemble_readout=True (the votes are taken from the logits the ensemble launch reads)")
        if rule not in _lib.EXIT_RULES:
            raise ValueError(f"rule must be one of {sorted(_lib.EXIT_RULES)}, got {rule!r}")
        if not 1 <= int(T) <= self.chunk_samples:
            raise ValueError(f"early exiting needs all T={T} samples in one chunk (engine planned for {self.chunk_samples})")
        B, T, first_exit = x.shape[0], int(T), int(first_exit)
        stages = self.exit_stages(first_exit)
        Q = QH = None
        if ensemble_readout:
            S, H, Q, QH = self.new_ensemble_sums(B)
        else:
            S, H = self.new_uncertainty_sums(B) if uncertainty else (self.new_moments(B), None)
        V = self.new_vote_counts(B) if votes else None
        exit_layer, active = self.accumulate_early_exit(x, S, T, threshold, seed, cnt0, first_exit, rule, ensemble, H, Q, QH, V)
        r = self.finalize(S, T) if H is None else self.finalize_uncertainty(S, H, T)
        r["exit_layer"] = exit_layer
        r["active_after"] = active
        idx = torch.arange(B, device=self.device)
        if ensemble_readout:
            r.update(self._finalize_ensemble_sums(Q, QH, T))
            at = exit_layer.long()
            r["best_ens"] = {k: r["ens_" + k][at, idx] for k in ("mean", "var", "pred_entropy", "exp_entropy", "mutual_info")}
        if votes:
            r.update(self.finalize_votes(V))
            r["V"] = V
        p = r["mean"]
        if ensemble and self.ensemble_weights is not None:      # the weighted mean of exits 0..e, in exit order (the rule's p)
            W, rows = self.ensemble_weights, []
            for e in range(self.n_exits):
                acc = torch.zeros_like(p[0])
                for i in range(e + 1):
                    acc = acc + float(W[e, i]) * p[i]
                rows.append(acc)
            p = torch.stack(rows)
        elif ensemble:        # the mean of exits 0..e, summed in exit order
            p = p.cumsum(0) / torch.arange(1, self.n_exits + 1, dtype=torch.float64, device=self.device).view(-1, 1, 1)
        r["best_preds"] = p[exit_layer.long(), idx]
        # images that ran stage k: all for stage 0, then those still active after exit first_exit + k - 1's test
        ran = [B] + [active[first_exit + k - 1] for k in range(1, len(stages))]
        done = 0
        for k, st in enumerate(stages):
            if ran[k] == 0:
                break
            done += ran[k] * (st["prefix_macs"] - st["whole_batch_macs"] + T * st["suffix_macs"]) + B * st["whole_batch_macs"]
        r["macs_done"] = done
        r["macs_full"] = B * (self.prefix_macs + T * self.suffix_macs)
        return r

    def accumulate_adaptive(self, x, S, T_max, threshold, rule="sem", t_step=None, test_exit=-1, seed=0, cnt0=0, H=None, image_offset=0,
                            ensemble=False, stop_on="exit", Q=None, QH=None, V=None):
        """The sampling half of ``predict_adaptive`` (bmi_forward_mcd_adaptive) into the ZEROED sums S [3, E, B, C] (and H [E, B]:
        ``new_uncertainty_sums``): on return image b's rows hold exactly its first t_used[b] samples.  With ``ensemble`` also into the
        ZEROED exit-ensemble sums ``Q`` [2, E, B, C] and ``QH`` [E, B] (``new_ensemble_sums``; H is required then), truncated the same way
        (bmi_forward_mcd_adaptive_ensemble); ``stop_on="ensemble"`` makes the rule read the ensemble of exits 0..test_exit (Q) in place of
        exit test_exit's own sums.  With ``V`` (ZEROED: ``new_vote_counts``; needs ``ensemble``) also the vote counts, truncated the same
        way: image b's rows are ``accumulate_votes``' over its first t_used[b] samples (bmi_forward_mcd_adaptive_votes).  Only then
        ``rule="votes"`` is allowed: ``threshold`` is the integer slack >= 0, and an image retires after t samples when no class can reach
        the leader of row test_exit of V[0] (``stop_on="exit"``) or V[1] (``"ensemble"``) in the T_max - t - slack samples still to come —
        with slack 0 its majority vote there is the full T_max run's, exactly; converged is then all ones.
        Returns (t_used int32 [B], converged uint8 [B], active_after_step host list)."""
        check_stop_on(stop_on, ensemble)
        x = self._check_x(x)
        B = x.shape[0]
        if V is not None and not ensemble:
            raise ValueError("the vote counts V need ensemble=True (the votes are taken from the logits the ensemble launch reads)")
        rules = _lib.STOP_RULES if V is None else _lib.VOTE_STOP_RULES
        if rule not in rules:
            raise ValueError(f"rule must be one of {sorted(rules)}, got {rule!r}" + (" (rule='votes' needs V)" if rule == "votes" else ""))
        if rule == "votes" and not (float(threshold) >= 0 and float(threshold) == int(float(threshold))):
            raise ValueError(f"rule='votes' takes a whole-number slack >= 0 as its threshold, got {threshold!r}")
        if t_step is None:
            t_step = min(DEFAULT_ADAPTIVE_T_STEP, self.chunk_samples)
        T_max, t_step, test_exit = int(T_max), int(t_step), int(test_exit)
        if T_max < 1:
            raise ValueError(f"T_max must be >= 1, got {T_max}")
        if not 1 <= t_step <= self.chunk_samples:
            raise ValueError(f"t_step must be in [1, {self.chunk_samples}] (the engine's planned chunk), got {t_step}")
        if test_exit < 0:
            test_exit += self.n_exits
        if not 0 <= test_exit < self.n_exits:
            raise ValueError(f"test_exit out of range for {self.n_exits} exits")
        if not ensemble and (Q is not None or QH is not None):
            raise ValueError("Q / QH are the sums of ensemble=True")
        self._check_sums(B, S, H, Q, QH, ensemble=ensemble)
        if V is not None:
            check_buffer(V, (2, self.n_exits, B, self.out_dim), torch.int32, self.device, "vote counts V")
        t_used = torch.empty(B, dtype=torch.int32, device=self.device)
        converged = torch.empty(B, dtype=torch.uint8, device=self.device)
        active = (C.c_int32 * (-(-T_max // t_step)))()
        name = "bmi_forward_mcd_adaptive_votes" if V is not None else "bmi_forward_mcd_adaptive_ensemble" if ensemble else "bmi_forward_mcd_adaptive"
        scratch = self._ensemble_scratch() if ensemble else None
        stop = (_lib.STOP_ON[stop_on],) if ensemble else ()
        votes = () if V is None else (V.data_ptr(), self._nonfinite.data_ptr())
        ens = (Q[0].data_ptr(), Q[1].data_ptr(), QH.data_ptr(), *votes, scratch.data_ptr(), scratch.numel()) if ensemble else ()
        with torch.cuda.device(self.device):
            rc = getattr(self.lib, name)(self.handle, x.data_ptr(), B, int(image_offset), T_max, t_step, int(seed) & 0xFFFFFFFFFFFFFFFF, int(cnt0),
                                         rules[rule], float(threshold), test_exit, *stop, S[0].data_ptr(), S[1].data_ptr(), S[2].data_ptr(),
                                         None if H is None else H.data_ptr(), *ens, t_used.data_ptr(), converged.data_ptr(), active,
                                         self.workspace.data_ptr(), self.workspace_bytes, self._stream())
        _lib.check(rc, name)
        return t_used, converged, [int(v) for v in active]

    def predict_adaptive(self, x, T_max, threshold, rule="sem", t_step=None, test_exit=-1, seed=0, cnt0=0, uncertainty=False,
                         image_offset=0, ensemble=False, stop_on="exit", votes=False):
        """Adaptive Monte-Carlo sampling on the device (bmi_forward_mcd_adaptive): samples run in steps of ``t_step`` (default
        DEFAULT_ADAPTIVE_T_STEP, at most the planned chunk) up to ``T_max``; after each step an image whose running estimate at exit
        ``test_exit`` passes the stop rule retires, and the later steps run on the images still active only.  Rules: ``"sem"`` — the
        largest standard error of the mean softmax, max_c sqrt(var_c / t), is at most ``threshold``; ``"margin"`` —
        (m_top1 - m_top2) / sqrt((var_top1 + var_top2) / t) is at least ``threshold``.  Every sample keeps its global index, so image b's
        result is ``predict(T=t_used[b])``'s for that image.  Returns dict(mean / var / logit_mean [E,B,C] float64, t_used int32 [B] and
        converged bool [B] on the device, active_after_step: host list of the images still active after each step); with
        ``uncertainty``, also pred_entropy / exp_entropy / mutual_info [E,B] as in ``finalize_uncertainty``.  With ``ensemble``, those
        entropies and the exit-ensemble read-out as well: the five ``ens_*`` entries of ``finalize_ensemble``, each image's divided by its own
        t_used[b], plus the sums ``Q`` [2, E, B, C] and ``QH`` [E, B] — image b's are ``predict_ensemble(T=t_used[b])``'s; and
        ``stop_on="ensemble"`` (needs ``ensemble``) tests the rule on the ensemble of exits 0..test_exit, the predictor a caller of the
        ensemble uses, instead of on exit test_exit alone.  With ``votes`` (needs ``ensemble``) also the eight entries of
        ``finalize_votes`` (no t_used needed: they divide by the votes cast) and the counts ``V`` [2, E, B, C] — image b's are
        ``predict_votes(T=t_used[b])``'s — and ``rule="votes"`` is allowed: ``threshold`` is then the integer slack (``accumulate_adaptive``).
        Synchronises once per step."""
        check_stop_on(stop_on, ensemble)
        if votes and not ensemble:
            raise ValueError("votes=True needs ensemble=True (the votes are taken from the logits the ensemble launch reads)")
        B = x.shape[0]
        Q = QH = None
        if ensemble:
            S, H, Q, QH = self.new_ensemble_sums(B)
        else:
            S, H = self.new_uncertainty_sums(B) if uncertainty else (self.new_moments(B), None)
        V = self.new_vote_counts(B) if votes else None
        t_used, converged, active = self.accumulate_adaptive(x, S, T_max, threshold, rule, t_step, test_exit, seed, cnt0, H, image_offset,
                                                             ensemble, stop_on, Q, QH, V)
        r = self.finalize_per_image(S, t_used, H)
        if ensemble:
            r.update(self.finalize_ensemble_per_image(Q, QH, t_used))
            r.update(Q=Q, QH=QH)
        if votes:
            r.update(self.finalize_votes(V))
            r["V"] = V
        r.update(t_used=t_used, converged=converged.bool(), active_after_step=active)
        return r

    def finalize_per_image(self, S, t_used, H=None):
        """``finalize`` (and, with H, ``finalize_uncertainty``) with image b's sums divided by its own sample count t_used[b]
        (bmi_finalize_per_image; device int32 [B], every entry >= 1)."""
        _, E, B, Cd = check_buffer(S, (3, None, None, None), torch.float64, self.device, "moment buffer S").shape
        check_buffer(t_used, (B,), torch.int32, self.device, "t_used")
        if H is not None:
            check_buffer(H, (E, B), torch.float64, self.device, "entropy buffer H")
        out = torch.empty_like(S)
        unc = None if H is None else torch.empty(3, E, B, dtype=torch.float64, device=S.device)
        ptr = (lambda i: None) if unc is None else (lambda i: unc[i].data_ptr())
        with torch.cuda.device(self.device):
            rc = self.lib.bmi_finalize_per_image(E, B, Cd, t_used.data_ptr(), S[0].data_ptr(), S[1].data_ptr(), S[2].data_ptr(),
                                                 None if H is None else H.data_ptr(), out[0].data_ptr(), out[1].data_ptr(), out[2].data_ptr(),
                                                 ptr(0), ptr(1), ptr(2), self._nonfinite.data_ptr(), self._stream())
        _lib.check(rc, "bmi_finalize_per_image")
        r = dict(mean=out[0], var=out[1], logit_mean=out[2])
        if unc is not None:
            r.update(pred_entropy=unc[0], exp_entropy=unc[1], mutual_info=unc[2])
        return r

    def forward_once(self, x, seed=0, t=0, cnt0=0):
        """One stochastic pass -> list of fp32 logits [B, C] per exit (the reference forward's return)."""
        S = self.new_moments(x.shape[0])
        self.accumulate(x, S, t, 1, seed, cnt0)
        return [S[2, e].float() for e in range(self.n_exits)]

    def forward_samples(self, x, T, seed=0, t_begin=0, cnt0=0, mask_stride=1, out=None):
        """Per-sample logits of the folded path (bmi_forward_mcd_samples): fp32 [T, E, B, C] — what T calls of the reference's
        ``model(x)`` return, from ONE pass of the engine over the batch (prefix once, the samples folded into the launches).
        ``mask_stride``: the Masksembles mask of sample i is (cnt0 + i * mask_stride) mod M (the reference's layers count forward
        calls: ``train/evaluate.py`` folds the T passes of batch k of an n-batch loader with cnt0 = cnt + k, mask_stride = n)."""
        x = self._check_x(x)
        B = x.shape[0]
        if out is None:
            out = torch.empty(T, self.n_exits, B, self.out_dim, dtype=torch.float32, device=self.device)
        else:
            check_buffer(out, (T, self.n_exits, B, self.out_dim), torch.float32, self.device, "out [T, E, B, C]")
        with torch.cuda.device(self.device):
            rc = self.lib.bmi_forward_mcd_samples(self.handle, x.data_ptr(), B, int(t_begin), int(T), int(seed) & 0xFFFFFFFFFFFFFFFF, int(cnt0),
                                                  int(mask_stride), out.data_ptr(), None, None, None, self.workspace.data_ptr(), self.workspace_bytes,
                                                  self._stream())
        _lib.check(rc, "bmi_forward_mcd_samples")
        return out

    def _sums_out(self, out, shape, name):
        """``out`` checked, or zeros when None: the float64 device sums an objective below ADDS into."""
        if out is None:
            return torch.zeros(*shape, dtype=torch.float64, device=self.device)
        return check_buffer(out, shape, torch.float64, self.device, name)

    def _nll_args(self, logits, labels):
        """What the three objectives below start from: (T, E, B, C) of the checked ``logits`` fp32 [T, E, B, C], and ``labels`` [B] as a
        device int32 tensor."""
        T, E, B, Cd = check_buffer(logits, (None,) * 4, torch.float32, self.device, "logits [T, E, B, C]").shape
        # (labels may come from the host in any integer type: converted first, so of the check below only the shape can fail)
        labels = check_buffer(labels.to(device=self.device, dtype=torch.int32).contiguous(), (B,), torch.int32, self.device, "labels [B]")
        return T, E, B, Cd, labels

    def nll_grid(self, logits, labels, tau_grid, out=None):
        """The objective of a temperature fit on the device (bmi_nll_temperature_grid): ``logits`` fp32 [T, E, B, C] (``forward_samples``),
        ``labels`` int [B] in [0, C) (the CALLER checks the range: ``train.calibration`` does, on the host), ``tau_grid`` [E, G] candidate
        temperatures.  ADDS, per exit and candidate, sum_b -log mean_t softmax(l_tb / tau)[y_b] into ``out`` (float64 [E, G], zeros when None)
        and returns it: a walk over a loader accumulates.  float64 throughout, log-sum-exp form, the same bits on every run;
        ``train.calibration.nll_grid_numpy`` is its host restatement.  Independent of the temperature set on this engine."""
        T, E, B, Cd, labels = self._nll_args(logits, labels)
        tau_grid = check_buffer(torch.as_tensor(tau_grid, dtype=torch.float32).to(self.device).contiguous(), (E, None), torch.float32, self.device,
                                "tau_grid [E, G]")
        G = tau_grid.shape[1]
        out = self._sums_out(out, (E, G), "out [E, G]")
        scratch = self._scratch("_nll_scratch", int(self.lib.bmi_nll_temperature_scratch_bytes(E, B, G)))
        with torch.cuda.device(self.device):
            rc = self.lib.bmi_nll_temperature_grid(logits.data_ptr(), T, E, B, Cd, labels.data_ptr(), tau_grid.data_ptr(), G, out.data_ptr(),
                                                   scratch.data_ptr(), scratch.numel(), self._stream())
        _lib.check(rc, "bmi_nll_temperature_grid")
        return out

    def _nll_map_grad(self, stem, name, rank, logits, labels, first, bias, out):
        """``nll_vector_grad`` (``rank`` 1: ``first`` is the scale [E, C]) and ``nll_matrix_grad`` (``rank`` 2: the matrix [E, C, C]):
        bmi_nll_<stem>_scaling_grad with bmi_nll_<stem>_scratch_bytes; ``name`` is what the messages call ``first``."""
        T, E, B, Cd, labels = self._nll_args(logits, labels)
        lead, dims = (E,) + (Cd,) * rank, "[E" + ", C" * rank + "]"
        first = check_buffer(torch.as_tensor(first, dtype=torch.float64).to(self.device).contiguous(), lead, torch.float64, self.device, f"{name} {dims}")
        bias = check_buffer(torch.as_tensor(bias, dtype=torch.float64).to(self.device).contiguous(), (E, Cd), torch.float64, self.device, "bias [E, C]")
        shapes = ((E,), lead, (E, Cd))
        names = ("nll [E]", f"g_{name} {dims}", "g_bias [E, C]")
        if out is None:
            out = tuple(torch.zeros(*shape, dtype=torch.float64, device=self.device) for shape in shapes)
        elif len(out) != 3:
            raise ValueError(f"out must be ({', '.join(names)})")
        else:
            for i, (o, shape) in enumerate(zip(out, shapes)):
                check_buffer(o, shape, torch.float64, self.device, f"out[{i}] ({names[i]})")
        scratch = self._scratch("_nll_scratch", int(getattr(self.lib, f"bmi_nll_{stem}_scratch_bytes")(E, B, Cd)))
        entry = f"bmi_nll_{stem}_scaling_grad"
        with torch.cuda.device(self.device):
            rc = getattr(self.lib, entry)(logits.data_ptr(), T, E, B, Cd, labels.data_ptr(), first.data_ptr(), bias.data_ptr(), out[0].data_ptr(),
                                          out[1].data_ptr(), out[2].data_ptr(), scratch.data_ptr(), scratch.numel(), self._stream())
        _lib.check(rc, entry)
        return out

    def nll_vector_grad(self, logits, labels, scale, bias, out=None):
        """Value and gradient of a vector-scaling fit on the device (bmi_nll_vector_scaling_grad): ``logits`` / ``labels`` as ``nll_grid``'s,
        ``scale`` / ``bias`` float64 [E, C] (arrays or tensors; taken as float64: the optimiser's point, not the head's float32).  ADDS, per
        exit, sum_b -log mean_t softmax(l_tb * scale + bias)[y_b] and its gradients into ``out`` = (nll [E], g_scale [E, C], g_bias [E, C]),
        device float64 (zeros when None), and returns the triple: a walk over a loader accumulates.  float64 throughout, the same bits on
        every run; ``train.calibration.nll_vector_numpy`` is its host restatement.  Independent of what is set on this engine."""
        return self._nll_map_grad("vector", "scale", 1, logits, labels, scale, bias, out)

    def nll_matrix_grad(self, logits, labels, matrix, bias, out=None):
        """Value and gradient of a matrix-scaling fit on the device (bmi_nll_matrix_scaling_grad): ``logits`` / ``labels`` as ``nll_grid``'s,
        ``matrix`` float64 [E, C, C] (row = output class) and ``bias`` float64 [E, C] (arrays or tensors; taken as float64: the optimiser's
        point, not the head's float32).  ADDS, per exit, sum_b -log mean_t softmax(M l_tb + bias)[y_b] and its gradients into ``out`` =
        (nll [E], g_matrix [E, C, C], g_bias [E, C]), device float64 (zeros when None), and returns the triple: a walk over a loader
        accumulates.  float64 throughout, the same bits on every run; ``train.calibration.nll_matrix_numpy`` is its host restatement.
        Independent of what is set on this engine."""
        return self._nll_map_grad("matrix", "matrix", 2, logits, labels, matrix, bias, out)

    def ensemble_nll_grid(self, logits, labels, tau, vary, cand, out=None):
        """The objective of a joint temperature fit of the exit ensembles on the device (bmi_nll_ensemble_temperature_grid): ``logits`` /
        ``labels`` as ``nll_grid``'s, ``tau`` the current temperatures (one per exit, a scalar for all, None for ones), ``vary`` the exits
        that take the candidate instead (an exit index, an iterable of indices, or None), ``cand`` [G] candidate temperatures.  ADDS, per
        row e and candidate, the NLL of the mean over exits 0..e and the T samples of the tempered softmax into ``out`` (float64 [E, G],
        zeros when None) and returns it.  One index is a coordinate step, every index one shared temperature, None with G = 1 evaluates
        ``tau``.  float64 throughout, the same bits on every run; ``train.calibration.ensemble_nll_grid_numpy`` is its host restatement.
        Independent of the temperature set on this engine."""
        T, E, B, Cd, labels = self._nll_args(logits, labels)
        tau = check_temperature(1.0 if tau is None else tau, E)
        mask = vary_mask(vary, E)
        tau = torch.tensor(tau, dtype=torch.float32).to(self.device)
        cand = check_buffer(torch.as_tensor(cand, dtype=torch.float32).to(self.device).contiguous(), (None,), torch.float32, self.device, "cand [G]")
        if cand.numel() < 1:
            raise ValueError("cand must be [G], G >= 1")
        G = cand.numel()
        out = self._sums_out(out, (E, G), "out [E, G]")
        scratch = self._scratch("_nll_scratch", int(self.lib.bmi_nll_ensemble_temperature_scratch_bytes(E, B, G)))
        with torch.cuda.device(self.device):
            rc = self.lib.bmi_nll_ensemble_temperature_grid(logits.data_ptr(), T, E, B, Cd, labels.data_ptr(), tau.data_ptr(), mask, cand.data_ptr(),
                                                            G, out.data_ptr(), scratch.data_ptr(), scratch.numel(), self._stream())
        _lib.check(rc, "bmi_nll_ensemble_temperature_grid")
        return out

    def pass_accuracy(self, logits, labels, tops=(1, 5), out=None, nonfinite=None):
        """Per-pass multi-exit accuracy on the device (bmi_pass_accuracy): ``logits`` fp32 [T, E, B, C] (``forward_samples``), ``labels`` int
        [B], ``tops`` the top-k cut-offs (at most 8, each >= 1).  Returns ``(hits, maxprob)``, device tensors: ``hits`` int32 [T, 2, E, K] —
        ``hits[t, 0, e, i]`` images of pass t whose label is among exit e's ``tops[i]`` highest logits, ``hits[t, 1, e, i]`` the same for the
        summed softmax of exits 0..e (ties go to the lower class index) — and ``maxprob`` float64 [T, E], the exits' max-probabilities summed
        over the images in image order.  Both are OVERWRITTEN (``out=(hits, maxprob)``: the caller's buffers, e.g. a row of its table).
        ``nonfinite``: an int32 [1] device counter the number of (pass, exit, image) rows with a non-finite logit is ADDED to (such a row is
        a miss and adds 0.0); a label outside [0, C) is a miss everywhere.  Exact counts, the same bits on every run;
        ``train.evaluate.pass_accuracy_numpy`` is its host restatement.  Raw logits: independent of what is set on this engine."""
        T, E, B, Cd, labels = self._nll_args(logits, labels)
        tops = [int(k) for k in tops]
        K = len(tops)
        if out is None:
            out = (torch.empty(T, 2, E, K, dtype=torch.int32, device=self.device), torch.empty(T, E, dtype=torch.float64, device=self.device))
        elif len(out) != 2:
            raise ValueError("out must be (hits [T, 2, E, K], maxprob [T, E])")
        else:
            check_buffer(out[0], (T, 2, E, K), torch.int32, self.device, "out[0] (hits [T, 2, E, K])")
            check_buffer(out[1], (T, E), torch.float64, self.device, "out[1] (maxprob [T, E])")
        if nonfinite is not None:
            check_buffer(nonfinite, (1,), torch.int32, self.device, "nonfinite [1]")
        scratch = self._scratch("_nll_scratch", int(self.lib.bmi_pass_accuracy_scratch_bytes(T, E, B)))
        with torch.cuda.device(self.device):
            rc = self.lib.bmi_pass_accuracy(logits.data_ptr(), T, E, B, Cd, labels.data_ptr(), (C.c_int32 * max(K, 1))(*tops), K, out[0].data_ptr(),
                                            out[1].data_ptr(), None if nonfinite is None else nonfinite.data_ptr(), scratch.data_ptr(),
                                            scratch.numel(), self._stream())
        _lib.check(rc, "bmi_pass_accuracy")
        return out

    # ---- reliability tables (bmi_reliability_record / bmi_reliability_table) -----------------------------------------------------
    def new_reliability_records(self, capacity, n_exits=None):
        """The record buffers of ``capacity`` images for ``reliability_records``: dict(keys int32 [R, capacity] — the float32 bit patterns
        of the confidences —, hit uint8, nll, brier float64 [R, capacity], counters int32 [2] = (non-finite rows, bad labels), zeroed),
        R = 2 * n_exits rows: the exits, then the exit ensembles.  21 bytes per row and image."""
        R, cap = 2 * int(self.n_exits if n_exits is None else n_exits), int(capacity)
        if R < 2 or cap < 1:
            raise ValueError("new_reliability_records needs n_exits >= 1 and capacity >= 1")
        return self._reliability_record_dict(R, cap)

    def _reliability_record_dict(self, R, cap):
        z = lambda *shape, dtype: torch.zeros(*shape, dtype=dtype, device=self.device)
        return dict(keys=z(R, cap, dtype=torch.int32), hit=z(R, cap, dtype=torch.uint8), nll=z(R, cap, dtype=torch.float64),
                    brier=z(R, cap, dtype=torch.float64), counters=z(2, dtype=torch.int32))

    # what the record and table calls of the read-outs check alike, the messages as their callers had them
    def _mean_labels(self, mean, labels):
        """(E, B, C, labels int32 [B] on the device) of a record call over ``mean`` [E, B, C]"""
        E, B, Cd = check_buffer(mean, (None,) * 3, torch.float64, self.device, "mean [E, B, C]").shape
        labels = check_buffer(labels.to(device=self.device, dtype=torch.int32).contiguous(), (B,), torch.int32, self.device, "labels [B]")
        return E, B, Cd, labels

    def _record_fit(self, R, cap, E, B, offset, Cr=None, Cd=None):
        """The offset of a record call whose batch fits records of R rows (and Cr classes, against the mean's Cd) and capacity ``cap``"""
        offset = int(offset)
        if R != 2 * E:
            raise ValueError(f"records hold {R} rows, mean has {E} exits (2 * E rows)")
        if Cr != Cd:
            raise ValueError(f"records hold {Cr} classes, mean has {Cd}")
        return self._check_fits(offset, B, cap)

    @staticmethod
    def _check_fits(offset, B, cap, empty_ok=True):
        offset = int(offset)
        if (B < 1 and not empty_ok) or offset < 0 or offset + B > cap:
            raise ValueError(f"images {offset} .. {offset + B - 1} do not fit the records' capacity {cap}")
        return offset

    @staticmethod
    def _check_n(n, cap, what="the records' capacity"):
        n = int(n)
        if not 1 <= n <= cap:
            raise ValueError(f"n = {n} outside [1, {cap}] ({what})")
        return n

    @staticmethod
    def _bin_edges(binning, n_bins, edges=None, allowed=("mass", "width")):
        """(n_bins, the host edges float32 [n_bins + 1] as a ctypes array, or None by mass) of a table call"""
        if binning not in allowed:
            raise ValueError("binning must be " + ", ".join(repr(b) for b in allowed[:-1]) + f" or {allowed[-1]!r}, got {binning!r}")
        fixed = None
        if binning == "edges":
            if edges is None:
                raise ValueError("binning 'edges' needs edges [n_bins + 1]")
            fixed = np.asarray(edges.detach().cpu() if torch.is_tensor(edges) else edges, dtype=np.float32).reshape(-1)
            n_bins = fixed.shape[0] - 1
            if n_bins >= 1 and (not np.isfinite(fixed).all() or (np.diff(fixed) < 0).any()):
                raise ValueError("edges must be finite and non-decreasing")
        n_bins = int(n_bins)
        if not 1 <= n_bins <= _lib.REL_MAX_BINS:
            raise ValueError(f"n_bins must be in [1, {_lib.REL_MAX_BINS}]")
        if binning == "width":
            fixed = np.arange(n_bins + 1, dtype=np.float32) / np.float32(n_bins)
        return n_bins, None if fixed is None else (C.c_float * (n_bins + 1))(*[float(v) for v in fixed])

    def _raise_counters(self, records, noun):
        nonfinite, badlabel = (int(v) for v in records["counters"].tolist())
        if nonfinite:
            raise FloatingPointError(f"{nonfinite} {noun} records with a non-finite probability on the {self.dtype!r} engine")
        if badlabel:
            raise ValueError(f"{badlabel} images with a label outside [0, C) in the {noun} records")

    def _check_records(self, records):
        R, cap = check_buffer(records["keys"], (None, None), torch.int32, self.device, "records['keys'] [R, capacity]").shape
        check_buffer(records["hit"], (R, cap), torch.uint8, self.device, "records['hit'] [R, capacity]")
        check_buffer(records["nll"], (R, cap), torch.float64, self.device, "records['nll'] [R, capacity]")
        check_buffer(records["brier"], (R, cap), torch.float64, self.device, "records['brier'] [R, capacity]")
        check_buffer(records["counters"], (2,), torch.int32, self.device, "records['counters'] [2]")
        return R, cap

    def reliability_records(self, mean, labels, records, offset):
        """Writes the reliability records of one batch on the device (bmi_reliability_record): ``mean`` float64 [E, B, C] (``finalize``'s
        T-mean probabilities), ``labels`` int [B], into columns ``offset .. offset + B - 1`` of ``records`` (``new_reliability_records``).
        Per exit and per exit ensemble (the mean of exits 0..e) and image: the float32 confidence of the arg-max (lowest index on ties)
        as its bit pattern, whether it hits the label, -log p_label and the Brier term.  A non-finite row or a label outside [0, C) leaves
        zeros and counts in ``records['counters']``.  One launch, no synchronisation; returns ``offset + B``.
        ``train.reliability.reliability_numpy`` is the host restatement."""
        E, B, Cd, labels = self._mean_labels(mean, labels)
        R, cap = self._check_records(records)
        offset = self._record_fit(R, cap, E, B, offset)
        with torch.cuda.device(self.device):
            rc = self.lib.bmi_reliability_record(mean.data_ptr(), E, B, Cd, labels.data_ptr(), offset, cap, records["keys"].data_ptr(),
                                                 records["hit"].data_ptr(), records["nll"].data_ptr(), records["brier"].data_ptr(),
                                                 records["counters"].data_ptr(), self._stream())
        _lib.check(rc, "bmi_reliability_record")
        return offset + B

    def reliability_table(self, records, n, n_bins=15, binning="mass", check=True):
        """The reliability table of the first ``n`` images of ``records`` on the device (bmi_reliability_table): a dict of device tensors —
        ``edges`` float32 [R, n_bins + 1], ``count`` / ``hits`` / ``conf_fix`` int64 [R, n_bins] (images, correct images and the sum of
        confidence * 2^40 per bin, bins ``edges[i] < conf <= edges[i + 1]``), ``sums`` float64 [R, 2] with its columns ``nll_sum`` and
        ``brier_sum`` (added in image order) — and ``n``.  ``binning``: "mass" (the equal-mass edges of ``train.metrics.ece_hist_binary``:
        order statistics of the confidences) or "width" (edges i / n_bins).  Exact integers, the same bits on every run and for every
        cut of the images into ``reliability_records`` calls; ``train.reliability.table_metrics`` derives ECE, MCE, NLL, Brier and accuracy.
        ``check`` (a host read: synchronises; pass False under a graph capture): FloatingPointError if a record was non-finite,
        ValueError if a label was outside [0, C)."""
        R, cap = self._check_records(records)
        n = self._check_n(n, cap)
        n_bins, edges_in = self._bin_edges(binning, n_bins)
        edges = torch.empty(R, n_bins + 1, dtype=torch.float32, device=self.device)
        ints = torch.empty(3, R, n_bins, dtype=torch.int64, device=self.device)
        sums = torch.empty(R, 2, dtype=torch.float64, device=self.device)
        scratch = self._scratch("_nll_scratch", max(1, int(self.lib.bmi_reliability_scratch_bytes(R, n, n_bins))))
        with torch.cuda.device(self.device):
            rc = self.lib.bmi_reliability_table(records["keys"].data_ptr(), records["hit"].data_ptr(), records["nll"].data_ptr(),
                                                records["brier"].data_ptr(), R, n, cap, n_bins, edges_in, edges.data_ptr(), ints[0].data_ptr(),
                                                ints[1].data_ptr(), ints[2].data_ptr(), sums.data_ptr(), scratch.data_ptr(), scratch.numel(),
                                                self._stream())
        _lib.check(rc, "bmi_reliability_table")
        if check:
            self._raise_counters(records, "reliability")
        return dict(edges=edges, count=ints[0], hits=ints[1], conf_fix=ints[2], sums=sums, nll_sum=sums[:, 0], brier_sum=sums[:, 1], n=n)

    def reliability_kde(self, records, n, grid_points=2 ** 14, order=1, bw_scale=None, check=True):
        """The KDE-ECE of the first ``n`` images of ``records`` on the device (bmi_reliability_kde) — the reference's ``ECE`` column, the
        top-label KDE calibration error of ``train.metrics.ece_kde_binary`` with the triweight densities evaluated exactly — from the
        records' float32 confidences and hit bits: a dict of device tensors, ``ece_kde``, ``bw``, ``sd`` float64 [R], ``n_data``, ``n_hit``
        int64 [R], ``degenerate`` int32 [R], ``density`` float64 [R, 2, grid_points] (the density of the correct predictions' confidences
        and of all confidences on linspace(-0.6, 1.6, grid_points), zero outside (0, 1)).  ``order``: 1 or 2; ``bw_scale``: the bandwidth is
        the standard deviation of the correct predictions' confidences times it, default the reference's ``(2 n) ** -0.2``.  A row without
        data or with a zero denominator (no hit, one hit, equal hit confidences: the reference's NaN) has ``degenerate`` 1 and value 0.0.
        Three launches, no allocation beyond the outputs; the same bits on every run and for every cut of the images into
        ``reliability_records`` calls; ``train.reliability.reliability_kde_numpy`` is the host restatement.
        ``check`` (a host read: synchronises; pass False under a graph capture): ValueError naming the degenerate rows."""
        R, cap = self._check_records(records)
        n, G, order = self._check_n(n, cap), int(grid_points), int(order)
        if not _lib.KDE_MIN_GRID <= G <= _lib.KDE_MAX_GRID:
            raise ValueError(f"grid_points must be in [{_lib.KDE_MIN_GRID}, {_lib.KDE_MAX_GRID}]")
        if order not in (1, 2):
            raise ValueError(f"order must be 1 or 2, got {order}")
        scale = float(2 * n) ** -0.2 if bw_scale is None else float(bw_scale)
        if not (np.isfinite(scale) and scale > 0.0):
            raise ValueError(f"bw_scale must be finite and positive, got {scale}")
        f64 = torch.empty(3, R, dtype=torch.float64, device=self.device)
        i64 = torch.empty(2, R, dtype=torch.int64, device=self.device)
        degenerate = torch.empty(R, dtype=torch.int32, device=self.device)
        density = torch.empty(R, 2, G, dtype=torch.float64, device=self.device)
        with torch.cuda.device(self.device):
            rc = self.lib.bmi_reliability_kde(records["keys"].data_ptr(), records["hit"].data_ptr(), R, n, cap, G, order, scale, f64[0].data_ptr(),
                                              f64[1].data_ptr(), f64[2].data_ptr(), i64[0].data_ptr(), i64[1].data_ptr(), degenerate.data_ptr(),
                                              density.data_ptr(), self._stream())
        _lib.check(rc, "bmi_reliability_kde")
        if check:
            bad = [r for r, v in enumerate(degenerate.tolist()) if v]
            if bad:
                from .train.reliability import row_names
                names = row_names(R // 2) if R % 2 == 0 else [str(r) for r in range(R)]
                raise ValueError("degenerate KDE-ECE rows (no data, or fewer than two distinct correct confidences): " +
                                 ", ".join(names[r] for r in bad))
        return dict(ece_kde=f64[0], bw=f64[1], sd=f64[2], n_data=i64[0], n_hit=i64[1], degenerate=degenerate, density=density)

    # ---- classwise reliability tables (bmi_classwise_record / bmi_classwise_table) -------------------------------------------------
    def new_classwise_records(self, capacity, n_exits=None, out_dim=None):
        """The record buffers of ``capacity`` images for ``classwise_records``: dict(pkeys int32 [R, C, capacity] — the float32 bit patterns
        of EVERY class's confidence, filled with INVALID (all ones: -1) —, labels int32 [capacity], filled with -1, counters int32 [2] =
        (non-finite rows, bad labels), zeroed), R = 2 * n_exits rows: the exits, then the exit ensembles; C = out_dim.
        4 * R * C bytes per image (plus 4 for the label): 32 MB at 4 exits, 100 classes and 10 000 images."""
        R, cap = 2 * int(self.n_exits if n_exits is None else n_exits), int(capacity)
        Cd = int(self.out_dim if out_dim is None else out_dim)
        if R < 2 or cap < 1 or Cd < 1:
            raise ValueError("new_classwise_records needs n_exits >= 1, out_dim >= 1 and capacity >= 1")
        return dict(pkeys=torch.full((R, Cd, cap), -1, dtype=torch.int32, device=self.device),
                    labels=torch.full((cap,), -1, dtype=torch.int32, device=self.device),
                    counters=torch.zeros(2, dtype=torch.int32, device=self.device))

    def _check_classwise_records(self, records):
        R, Cd, cap = check_buffer(records["pkeys"], (None,) * 3, torch.int32, self.device, "records['pkeys'] [R, C, capacity]").shape
        check_buffer(records["labels"], (cap,), torch.int32, self.device, "records['labels'] [capacity]")
        check_buffer(records["counters"], (2,), torch.int32, self.device, "records['counters'] [2]")
        return R, Cd, cap

    def classwise_records(self, mean, labels, records, offset):
        """Writes the classwise records of one batch on the device (bmi_classwise_record): ``mean`` float64 [E, B, C] (``finalize``'s
        T-mean probabilities), ``labels`` int [B], into columns ``offset .. offset + B - 1`` of ``records`` (``new_classwise_records``).
        Per exit and per exit ensemble, image AND class: the float32 confidence p_c / sum p (zero below 2^-126) as its bit pattern — at
        the arg-max class the key ``reliability_records`` writes —, and the image's label.  A non-finite row or a label outside [0, C)
        leaves INVALID keys (a bad label: the label record -1) and counts in ``records['counters']``.  4 * R * C bytes per image.
        One launch, no synchronisation; returns ``offset + B``.  ``train.reliability.classwise_numpy`` is the host restatement."""
        E, B, Cd, labels = self._mean_labels(mean, labels)
        R, Cr, cap = self._check_classwise_records(records)
        offset = self._record_fit(R, cap, E, B, offset, Cr, Cd)
        with torch.cuda.device(self.device):
            rc = self.lib.bmi_classwise_record(mean.data_ptr(), E, B, Cd, labels.data_ptr(), offset, cap, records["pkeys"].data_ptr(),
                                               records["labels"].data_ptr(), records["counters"].data_ptr(), self._stream())
        _lib.check(rc, "bmi_classwise_record")
        return offset + B

    def classwise_table(self, records, n, n_bins=15, binning="width", edges=None, check=True):
        """The classwise reliability table of the first ``n`` images of ``records`` on the device (bmi_classwise_table): a dict of device
        tensors — ``edges`` float32 [R, C, n_bins + 1], ``count`` / ``hits`` / ``conf_fix`` int64 [R, C, n_bins] (per class the pairs
        (image, class), those whose label is the class, and the sum of the truncated confidence * 2^40 per bin; bin 0 is closed at its
        lower edge, so confidence zero is counted), ``valid`` int64 [R] (the images of the row that are data) — and ``n``.  ``binning``:
        "width" (edges i / n_bins: the published classwise ECE), "mass" (per (row, class) the order statistics of its confidences) or
        "edges" with the caller's ``edges`` [n_bins + 1] (finite, non-decreasing; ``edges[0] > 0`` ignores the negligible probabilities),
        which then sets ``n_bins``.  Exact integers, the same bits on every run and for every cut of the images into ``classwise_records``
        calls; ``train.reliability.classwise_metrics`` derives the classwise ECE.  Two launches, no allocation beyond the outputs.
        ``check`` (a host read: synchronises; pass False under a graph capture): FloatingPointError if a record was non-finite,
        ValueError if a label was outside [0, C)."""
        R, Cd, cap = self._check_classwise_records(records)
        n = self._check_n(n, cap)
        n_bins, edges_in = self._bin_edges(binning, n_bins, edges, ("mass", "width", "edges"))
        out_edges = torch.empty(R, Cd, n_bins + 1, dtype=torch.float32, device=self.device)
        ints = torch.empty(3, R, Cd, n_bins, dtype=torch.int64, device=self.device)
        valid = torch.empty(R, dtype=torch.int64, device=self.device)
        with torch.cuda.device(self.device):
            rc = self.lib.bmi_classwise_table(records["pkeys"].data_ptr(), records["labels"].data_ptr(), R, Cd, n, cap, n_bins, edges_in,
                                              out_edges.data_ptr(), ints[0].data_ptr(), ints[1].data_ptr(), ints[2].data_ptr(), valid.data_ptr(),
                                              self._stream())
        _lib.check(rc, "bmi_classwise_table")
        if check:
            self._raise_counters(records, "classwise")
        return dict(edges=out_edges, count=ints[0], hits=ints[1], conf_fix=ints[2], valid=valid, n=n)

    # ---- rank quality of the uncertainty scores (bmi_score_record / bmi_rank_quality) ---------------------------------------------
    def new_score_records(self, capacity, rows):
        """The key buffer of ``capacity`` images and ``rows`` rows for ``score_records``: dict(ukeys int32 [rows, capacity] — uint32 bit
        patterns, filled with INVALID (all ones: -1) —, counter int32 [1] = the scores that were NaN, infinite or negative, zeroed)."""
        R, cap = int(rows), int(capacity)
        if R < 1 or cap < 1:
            raise ValueError("new_score_records needs rows >= 1 and capacity >= 1")
        return dict(ukeys=torch.full((R, cap), -1, dtype=torch.int32, device=self.device),
                    counter=torch.zeros(1, dtype=torch.int32, device=self.device))

    def score_records(self, score, records, offset, direction, valid=None):
        """Writes the score keys of one batch on the device (bmi_score_record): ``score`` float64 [R, B], non-negative, into columns
        ``offset .. offset + B - 1`` of ``records`` (``new_score_records``).  The key is the float32 bit pattern of the score for
        ``direction=+1`` (an uncertainty: entropy, mutual information, variation ratio, vote entropy) and 0x7F7FFFFF minus it for
        ``direction=-1`` (a confidence): ascending unsigned key order is "most certain first".  A NaN, infinite or negative score gives
        INVALID (all ones) and counts in ``records['counter']``.  ``valid``: int32 [R, capacity], the reliability records' ``keys``; where it
        is 0 (a bad label, a non-finite row) the image is INVALID in that row and not counted here.  One launch, no synchronisation;
        returns ``offset + B``.  ``train.ranking.score_keys_numpy`` is the host restatement."""
        R, B = check_buffer(score, (None, None), torch.float64, self.device, "score [R, B]").shape
        cap = check_buffer(records["ukeys"], (R, None), torch.int32, self.device, "records['ukeys'] [R, capacity]").shape[1]
        check_buffer(records["counter"], (1,), torch.int32, self.device, "records['counter'] [1]")
        direction = int(direction)
        if direction not in (1, -1):
            raise ValueError(f"direction must be +1 (an uncertainty) or -1 (a confidence), got {direction}")
        offset = self._check_fits(offset, B, cap, empty_ok=False)
        if not (R <= _lib.RANK_MAX_ROWS and B <= _lib.RANK_MAX_IMAGES):
            raise ValueError(f"score_records takes at most {_lib.RANK_MAX_ROWS} rows and {_lib.RANK_MAX_IMAGES} images per call")
        if valid is not None:
            check_buffer(valid, (R, cap), torch.int32, self.device, "valid [R, capacity]")
        with torch.cuda.device(self.device):
            rc = self.lib.bmi_score_record(score.data_ptr(), R, B, direction, _ptr(valid), offset, cap, records["ukeys"].data_ptr(),
                                           records["counter"].data_ptr(), self._stream())
        _lib.check(rc, "bmi_score_record")
        return offset + B

    def rank_quality(self, ukeys, positive, n):
        """The rank quality of the first ``n`` images of ``ukeys`` int32 [R, capacity] (``score_records``) against ``positive`` uint8
        [R, capacity] — 1 where the image is what the score should flag: a wrong prediction, a noise image — on the device
        (bmi_rank_quality).  The valid images of a row (key not INVALID), m of them, stand in the stable ascending key order, most certain
        first, ties by image index.  A dict of device tensors: ``rank`` int32 [R, capacity] (the image's position, -1 for an invalid
        image), ``sorted_keys`` int32 [R, capacity] (position k: the key of the image ranked k, all ones from m on), ``curve`` int32
        [R, capacity] (position k: the positives at positions 0 .. k, n_pos from m on) — columns beyond ``n`` are zero —, ``counts`` int64
        [R, 3] = (m, n_pos, U2) with AUROC = U2 / (2 n_pos n_neg), ``aurc_sum`` float64 [R] = sum_k curve[k] / (k + 1) in position order —
        and ``n``.  Exact integers, O(n^2) compare steps per row and no sort; the same bits on every run and for every cut of the images
        into ``score_records`` calls.  ``train.ranking.rank_metrics`` derives AUROC, AURC and E-AURC; ``rank_quality_numpy`` restates it."""
        R, cap = check_buffer(ukeys, (None, None), torch.int32, self.device, "ukeys [R, capacity]").shape
        check_buffer(positive, (R, cap), torch.uint8, self.device, "positive [R, capacity]")
        n = self._check_n(n, cap, "the capacity")
        if n > _lib.RANK_MAX_IMAGES or R > _lib.RANK_MAX_ROWS:
            raise ValueError(f"rank_quality takes at most {_lib.RANK_MAX_IMAGES} images and {_lib.RANK_MAX_ROWS} rows (n = {n}, R = {R})")
        ints = torch.zeros(3, R, cap, dtype=torch.int32, device=self.device)
        counts = torch.empty(R, 3, dtype=torch.int64, device=self.device)
        aurc_sum = torch.empty(R, dtype=torch.float64, device=self.device)
        scratch = self._scratch("_nll_scratch", max(1, int(self.lib.bmi_rank_scratch_bytes(R, n))))
        with torch.cuda.device(self.device):
            rc = self.lib.bmi_rank_quality(ukeys.data_ptr(), positive.data_ptr(), R, n, cap, ints[0].data_ptr(), ints[1].data_ptr(),
                                           ints[2].data_ptr(), counts.data_ptr(), aurc_sum.data_ptr(), scratch.data_ptr(), scratch.numel(),
                                           self._stream())
        _lib.check(rc, "bmi_rank_quality")
        return dict(rank=ints[0], sorted_keys=ints[1], curve=ints[2], counts=counts, aurc_sum=aurc_sum, n=n)

    # ---- exit-policy sweep (bmi_exit_stat_record / bmi_exit_policy_sweep) ----------------------------------------------------------
    def new_exit_stat_records(self, capacity, n_exits=None):
        """The statistic buffer of ``capacity`` images for ``exit_stat_records``: dict(stat float64 [2, E, capacity], zeroed) — plane 0 the
        exits' own statistics, plane 1 the exit ensembles'.  16 bytes per exit and image."""
        E, cap = int(self.n_exits if n_exits is None else n_exits), int(capacity)
        if E < 1 or cap < 1:
            raise ValueError("new_exit_stat_records needs n_exits >= 1 and capacity >= 1")
        return dict(stat=torch.zeros(2, E, cap, dtype=torch.float64, device=self.device))

    def exit_stat_records(self, S, t_count, records, offset, rule="confidence"):
        """Writes the decision statistics of one batch on the device (bmi_exit_stat_record): ``S`` [3, E, B, C], the sums ``accumulate``
        filled over ``t_count`` samples (or S1 [E, B, C] alone), into columns ``offset .. offset + B - 1`` of ``records``
        (``new_exit_stat_records``).  ``stat[ens, e, n]`` is the very number ``predict_early_exit(rule=, ensemble=ens)`` compares with its
        threshold at exit e — S1 / t in the device rule's arithmetic, not ``finalize``'s mean S1 * (1 / t) —, under the engine's ensemble
        weights if set.  A NaN is stored as it is.  One launch, no synchronisation; returns ``offset + B``.
        ``train.exit_policy.exit_stat_numpy`` is the host restatement."""
        if rule not in _lib.EXIT_RULES:
            raise ValueError(f"rule must be one of {sorted(_lib.EXIT_RULES)}, got {rule!r}")
        S1 = S[0] if S.dim() == 4 else S
        E, B, Cd = check_buffer(S1, (None,) * 3, torch.float64, self.device, "S1 [E, B, C]").shape
        cap = check_buffer(records["stat"], (2, E, None), torch.float64, self.device, "records['stat'] [2, E, capacity]").shape[2]
        t_count = int(t_count)
        if t_count < 1:
            raise ValueError(f"t_count must be >= 1, got {t_count}")
        offset = self._check_fits(offset, B, cap, empty_ok=False)
        if E > 32 or Cd > 128:
            raise ValueError(f"exit_stat_records takes at most 32 exits and 128 classes (E = {E}, C = {Cd})")
        w = self._ens_w_dev if E == self.n_exits else None
        with torch.cuda.device(self.device):
            rc = self.lib.bmi_exit_stat_record(S1.data_ptr(), E, B, Cd, t_count, _lib.EXIT_RULES[rule], _ptr(w), offset, cap,
                                               records["stat"].data_ptr(), self._stream())
        _lib.check(rc, "bmi_exit_stat_record")
        return offset + B

    def exit_policy_sweep(self, stat_records, reliability_records, n, thresholds, ensemble=False, first_exit=1, select=False, exit_of=False):
        """The exit policy of every threshold over the first ``n`` images, on the device (bmi_exit_policy_sweep): ``stat_records`` from
        ``exit_stat_records``, ``reliability_records`` from ``reliability_records`` (the outcome at every exit and exit ensemble),
        ``thresholds`` a sequence or a float64 tensor [G], any order, G <= 1024.  Per threshold an image leaves at the lowest exit e in
        [first_exit, E-2] whose statistic exceeds it (strictly), else at the last: the exit ``predict_early_exit`` assigns.  ``ensemble``:
        the ensemble statistics decide and the equal-mean exit ensembles' outcome rows are read — ValueError while ensemble weights are
        set, because those rows are not the weighted ensemble's.  A dict of device tensors: ``count`` / ``hits`` int64 [G, E] (images
        leaving at each exit, the correct ones among them), ``invalid`` int64 [G] (images whose outcome record is empty: a bad label, a
        non-finite row; in no count), ``thresholds`` float64 [G], with ``exit_of`` also ``exit_of`` uint8 [G, capacity], with ``select``
        (G <= 64) also ``selected``: a record dict of G rows — the four records at the exit taken, zeros for an invalid image — that
        ``reliability_table`` / ``reliability_kde`` / ``score_records(valid=)`` take as they take ``reliability_records``' — and ``n``.
        Columns beyond ``n`` are zero.  Integers only; the same bits on every run and for every cut of the images into record calls.  A NaN
        threshold lets nobody leave early.  Two launches, no synchronisation.  ``train.exit_policy.exit_policy_numpy`` restates it."""
        R, cap = self._check_records(reliability_records)
        E = R // 2
        check_buffer(stat_records["stat"], (2, E, cap), torch.float64, self.device, "stat_records['stat'] [2, E, capacity]")
        if R != 2 * E:
            raise ValueError(f"reliability records of {R} rows are not 2 * E rows")
        if not torch.is_tensor(thresholds):
            thresholds = torch.as_tensor(np.asarray(thresholds, dtype=np.float64).reshape(-1))
        thr = check_buffer(thresholds.to(device=self.device, dtype=torch.float64).contiguous(), (None,), torch.float64, self.device, "thresholds [G]")
        G, n, first_exit, kind = thr.shape[0], self._check_n(n, cap), int(first_exit), int(bool(ensemble))
        if not 0 <= first_exit < E:
            raise ValueError(f"first_exit must be in [0, {E})")
        if not 1 <= G <= _lib.POLICY_MAX_THRESHOLDS:
            raise ValueError(f"exit_policy_sweep takes 1 .. {_lib.POLICY_MAX_THRESHOLDS} thresholds, got {G}")
        if select and G > _lib.POLICY_MAX_RECORD_ROWS:
            raise ValueError(f"select=True takes at most {_lib.POLICY_MAX_RECORD_ROWS} thresholds (the rows a reliability table takes), got {G}")
        if kind and self.ensemble_weights is not None:
            raise ValueError("the ensemble policy under ensemble weights: the reliability records' ensemble rows are the equal-mean ensemble's")
        ints = torch.empty(2, G, E, dtype=torch.int64, device=self.device)
        invalid = torch.empty(G, dtype=torch.int64, device=self.device)
        ex = torch.zeros(G, cap, dtype=torch.uint8, device=self.device) if exit_of else None
        sel = self._reliability_record_dict(G, cap) if select else None
        rec = reliability_records
        scratch = self._scratch("_nll_scratch", max(1, int(self.lib.bmi_exit_policy_scratch_bytes(E, n, G))))
        with torch.cuda.device(self.device):
            rc = self.lib.bmi_exit_policy_sweep(stat_records["stat"][kind].data_ptr(), E, n, cap, first_exit, thr.data_ptr(), G,
                                                rec["keys"][kind * E:].data_ptr(), rec["hit"][kind * E:].data_ptr(), rec["nll"][kind * E:].data_ptr(),
                                                rec["brier"][kind * E:].data_ptr(), ints[0].data_ptr(), ints[1].data_ptr(), invalid.data_ptr(),
                                                _ptr(ex), *((_ptr(sel[k]) for k in ("keys", "hit", "nll", "brier")) if select else (None,) * 4),
                                                scratch.data_ptr(), scratch.numel(), self._stream())
        _lib.check(rc, "bmi_exit_policy_sweep")
        out = dict(count=ints[0], hits=ints[1], invalid=invalid, thresholds=thr, n=n)
        if exit_of:
            out["exit_of"] = ex
        if select:
            out["selected"] = sel
        return out

    def exit_costs(self, T, first_exit=1):
        """What an image costs when it leaves at each exit under ``predict_early_exit(T=, first_exit=)``, from ``exit_stages`` (host only):
        dict(per_exit: a list of E Python ints, the cumulative MACs of the stages an image leaving at exit e ran — each stage's
        prefix MACs without its whole-batch ops plus T x its suffix MACs; 0 for the exits before ``first_exit``, where nobody leaves —,
        stage_macs / whole_batch_macs: the per-stage terms (whole-batch ops run over all B images whenever anybody reaches the stage),
        macs_full: ``predict``'s MACs per image, T, first_exit).  ``train.exit_policy.policy_macs`` turns a count row into
        ``predict_early_exit``'s ``macs_done``."""
        T, first_exit = int(T), int(first_exit)
        if T < 1:
            raise ValueError(f"T must be >= 1, got {T}")
        from .train.exit_policy import stage_costs
        costs = stage_costs(self.exit_stages(first_exit), T, first_exit, self.n_exits)
        costs["macs_full"] = int(self.prefix_macs + T * self.suffix_macs)
        return costs

    def read_tensor(self, tensor_id, batch, samples=1):
        """A copy of graph tensor ``tensor_id`` as it sits in the workspace after a forward (bmi_tensor_info): fp32
        [samples * batch or batch, h, w, c].  For per-layer traces (tools/layer_trace.py): plan the engine under
        ``set_option("ws_no_reuse", 1)`` (and ``mask_lazy`` = 0, ``conv_pool`` = 0), else a later tensor may have taken the range."""
        off, eb, ps = C.c_int64(), C.c_int32(), C.c_int32()
        th, tw, tc = C.c_int32(), C.c_int32(), C.c_int32()
        _lib.check(self.lib.bmi_tensor_info(self.handle, int(tensor_id), C.byref(off), C.byref(eb), C.byref(ps), C.byref(th),
                                            C.byref(tw), C.byref(tc)), "bmi_tensor_info")
        n = batch * (samples if ps.value & 1 else 1)
        count = n * th.value * tw.value * tc.value
        raw = self.workspace[off.value:off.value + count * eb.value]
        if ps.value & 2:                   # the split engines' pair32 layout: per pixel, 32-channel blocks [32 heads | 32 tails]
            dt16 = torch.bfloat16 if self.dtype == "bf16x3" else torch.float16
            blocks = raw.view(dt16).view(n, th.value, tw.value, tc.value // 32, 2, 32).float()
            return (blocks[..., 0, :] + blocks[..., 1, :]).reshape(n, th.value, tw.value, tc.value).clone()
        dt = torch.float32 if eb.value == 4 else (torch.bfloat16 if self.dtype == "bf16" else torch.float16)
        return raw.view(dt).view(n, th.value, tw.value, tc.value).float().clone()

    # ---- measurement helpers ---------------------------------------------------------------------
    profiling = False

    def profile(self, enable):
        _lib.check(self.lib.bmi_profile_enable(self.handle, int(bool(enable))), "bmi_profile_enable")
        self.profiling = bool(enable)

    def profile_read(self):
        ms = (C.c_double * _lib.PROFILE_SLOTS)()
        n = (C.c_int64 * _lib.PROFILE_SLOTS)()
        _lib.check(self.lib.bmi_profile_read(self.handle, ms, n), "bmi_profile_read")
        out = {_lib.PROFILE_NAMES.get(i, str(i)): (ms[i], n[i]) for i in range(_lib.PROFILE_SLOTS) if n[i]}
        nf = _lib.CONV_FAMILIES
        fms, fn, ffl, fby = (C.c_double * nf)(), (C.c_int64 * nf)(), (C.c_double * nf)(), (C.c_double * nf)()
        _lib.check(self.lib.bmi_profile_conv_families(self.handle, fms, fn, ffl, fby), "bmi_profile_conv_families")
        names = _lib.CONV_FAMILY_KERNELS
        self.conv_families = {names[i]: dict(ms=fms[i], launches=fn[i], flops=ffl[i], bytes=fby[i]) for i in range(nf) if fn[i]}
        return out

    def profile_launches(self):
        """The launches behind the last profile_read(), in order: dicts with kind, family, out (tensor id), images, ms, flops, bytes."""
        cnt = C.c_int32(0)
        _lib.check(self.lib.bmi_profile_launches(self.handle, 0, C.byref(cnt), None, None, None, None, None, None, None), "bmi_profile_launches")
        n = cnt.value
        ki, fa, ou, im = ((C.c_int32 * n)() for _ in range(4))
        ms, fl, by = ((C.c_double * n)() for _ in range(3))
        _lib.check(self.lib.bmi_profile_launches(self.handle, n, C.byref(cnt), ki, fa, ou, im, ms, fl, by), "bmi_profile_launches")
        names = [k[:-len("_kernel")] for k in _lib.CONV_FAMILY_KERNELS]
        return [dict(kind=_lib.PROFILE_NAMES.get(ki[i], str(ki[i])), family=names[fa[i]] if 0 <= fa[i] < len(names) else None, out=ou[i], images=im[i],
                     ms=ms[i], flops=fl[i], bytes=by[i]) for i in range(n)]


class BatchesInFlight:
    """`n` independent engines of one model (own workspace, own device copy of the weights) on `n` streams: consecutive batches
    alternate between them, so the launch-bound once-per-batch prefix of batch k+1 (five ~50 us launches on B images) runs
    beside the sample-folded suffix of batch k instead of in front of it.  Nothing changes inside a batch — every per-sample
    value and every float64 moment sum is bit for bit the single-stream one (the 32-sample groups of an image are joined
    in group order) — only the order in which the GPU sees the launches of neighbouring batches changes.  Measured on
    one MI355X (tools/experiments/two_batches.py), 1 -> 2 batches in flight: VGG-11 T=30 0.368 -> 0.297 ms per batch, ResNet-18
    Masksembles T=8 2.52 -> 2.23 ms, ResNet-18 multi-exit at T=13 (one rank's share of eight) 3.77 -> 3.34 ms, at T=100 24.19 ->
    23.76 ms.

        pipe = BatchesInFlight(model, device, n=2, max_batch=250)
        for x in batches:
            out = pipe.submit(lambda eng: eng.predict(x, T, seed))     # asynchronous; device tensors
        pipe.synchronize()
    """

    def __init__(self, model, device, n=2, **engine_kwargs):
        if n < 1:
            raise ValueError("n >= 1 batches in flight")
        self._model = model
        self.engines = [MCDEngine(model, device, **engine_kwargs) for _ in range(n)]
        self.device = self.engines[0].device
        self.streams = [torch.cuda.Stream(self.device) for _ in range(n)] if n > 1 else [None]
        self.last_stream = None
        self.last_engine = None
        self.k = 0

    def slot(self):
        return self.k % len(self.engines)

    use_graph = False      # step(): one hipGraph replay per batch step (tuned() sets it for launch-bound models)

    def close(self):
        """Destroys the engines and drops their workspaces, captured graphs and static buffers (a pipe that is being replaced by a larger
        one, or whose model's weights changed)."""
        self.synchronize()
        self._drop_graphs()
        for e in self.engines:
            e.close()
            e.workspace = None
            e.__dict__.pop("_step_S", None)
            e.__dict__.pop("_share_parts", None)
        self.engines = []

    @classmethod
    def tuned(cls, model, device, x, T, seed=0, cnt0=0, threshold_ms=1.5, allow_graph=True, group=None, **engine_kwargs):
        """The pipe a model should run with, decided by MEASUREMENT on its first batch: one engine is built, a batch step (x, T) is
        warmed up and timed with HIP events; a step under ``threshold_ms`` is launch-bound (VGG-11 at batch 250 x T = 30: ~20 launches of
        20-50 us on a ~20 us launch floor, 0.26 ms per step) and gets THREE batches in flight, each step ONE hipGraph replay
        (``predict_graphed``: 28 -> 38 M MCD-samples/s on VGG-11, round-3 measurement); anything longer (the ResNets at T = 100:
        21 ms) gets two eager engines, where a replay buys nothing and a third workspace costs memory.  ``pipe.step(x, T, seed)`` runs a
        batch either way; results are bit for bit the same in both modes (tests/test_gpu_model.py).  ``allow_graph=False``: a caller whose launch
        scalars change from batch to batch (FullAnalysis with MC-dropout sites: the batch index is part of the seed) takes the three batches in
        flight without the replay.  ``group``: the ranks of a process group time their SHARE of the step and decide together (MAX over ranks)."""
        pipe = cls(model, device, n=1, **engine_kwargs)
        from .sharding import _rank_world, accumulate_share
        rank, world = _rank_world(group) if group is not None else (0, 1)
        if world > 1:
            # a rank's SHARE of the step is what it will run; the group takes the slowest rank's figure so that every rank builds the same pipe
            import torch.distributed as dist
            S = pipe.engines[0].new_moments(x.shape[0])
            ms = pipe.measure_ms(lambda e: accumulate_share(e, x, S.zero_(), T, seed, cnt0, rank, world), warm=1, reps=2)
            on_dev = dist.get_backend(group) == "nccl"
            t = torch.tensor([ms], dtype=torch.float64, device=pipe.device if on_dev else "cpu")
            dist.all_reduce(t, op=dist.ReduceOp.MAX, group=group)
            ms = float(t.item())
        else:
            ms = pipe.measure_ms(lambda e: e.predict(x, T, seed, cnt0=cnt0), warm=1, reps=2)
        pipe.step_ms_measured = ms
        launch_bound = ms < threshold_ms
        pipe.grow(3 if launch_bound else 2)
        pipe.use_graph = bool(launch_bound and allow_graph)
        return pipe

    def measure_ms(self, fn, warm=2, reps=3):
        """Milliseconds per call of ``fn(engine 0)`` on the current stream (HIP events; ``warm`` untimed calls first)."""
        eng = self.engines[0]
        for _ in range(warm):
            fn(eng)
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
        ev[0].record(torch.cuda.current_stream(self.device))
        for _ in range(reps):
            fn(eng)
        ev[1].record(torch.cuda.current_stream(self.device))
        ev[1].synchronize()
        return ev[0].elapsed_time(ev[1]) / reps

    def grow(self, n):
        """``n`` batches in flight from now on: more engines of the same model (own workspace, own weights), one stream each."""
        if n < len(self.engines):
            raise ValueError("a pipe only grows")
        e0 = self.engines[0]
        kw = dict(max_batch=e0.max_batch, chunk_samples=e0.chunk_samples if e0.chunk_explicit else None, dtype=e0.dtype)
        self.engines += [MCDEngine(self._model, self.device, **kw) for _ in range(n - len(self.engines))]
        self.streams = [torch.cuda.Stream(self.device) for _ in range(n)] if n > 1 else [None]
        self._drop_graphs()
        return self

    def _drop_graphs(self):
        """Forgets the captured hipGraphs and their streams: a captured launch carries its kernel arguments and its instantiation."""
        for attr in ("_graphs", "_gstreams"):
            if hasattr(self, attr):
                delattr(self, attr)

    def _set_on_engines(self, setter, *args):
        self.synchronize()
        for e in self.engines:
            getattr(e, setter)(*args)
        self._drop_graphs()

    def set_temperature(self, tau):
        """``MCDEngine.set_temperature`` on every engine of the pipe; the captured hipGraphs are discarded (after a synchronize): a captured
        launch carries its kernel arguments and its instantiation, so a replay would run under the temperature it was captured with."""
        self._set_on_engines("set_temperature", tau)

    def set_vector_scaling(self, scale, bias=None):
        """``MCDEngine.set_vector_scaling`` on every engine of the pipe; the captured hipGraphs are discarded (after a synchronize), like
        ``set_temperature``'s: a replay would run the instantiation and the pointers it was captured with."""
        self._set_on_engines("set_vector_scaling", scale, bias)

    def set_matrix_scaling(self, matrix, bias=None):
        """``MCDEngine.set_matrix_scaling`` on every engine of the pipe; the captured hipGraphs are discarded (after a synchronize), like
        ``set_vector_scaling``'s."""
        self._set_on_engines("set_matrix_scaling", matrix, bias)

    def step(self, x, T, seed=0, cnt0=0, group=None, kind=None, shard=False):
        """One batch step on the next slot — a hipGraph replay (``use_graph``) or eager — with the work partitioned over ``group`` when
        one is given (``shard=True``: the default group).  Returns what ``MCDEngine.finalize`` returns (device tensors on ``last_stream``)."""
        if self.use_graph:
            return self.predict_graphed(x, T, seed, cnt0, group=group, kind=kind, shard=shard)
        from .sharding import accumulate_partitioned

        def run(e):
            S = e.__dict__.get("_step_S")
            if S is None or S.shape[2] != x.shape[0]:
                S = e.__dict__["_step_S"] = e.new_moments(x.shape[0])
            else:
                S.zero_()
            if group is not None or shard:
                accumulate_partitioned(e, x, S, T, seed, cnt0, group=group, kind=kind)
            else:
                e.accumulate(x, S, 0, T, seed, cnt0)
            return e.finalize(S, T)
        return self.submit(run, inputs=(x,))

    def submit(self, fn, inputs=()):
        """Runs fn(engine) on the next slot's stream (after everything already queued on the caller's current stream, which is
        where the inputs come from) and returns what it returns.  `inputs`: device tensors fn reads that the caller may drop
        before the batch has run (they are recorded on the stream so the caching allocator does not hand their memory out
        early).  The results are produced on `self.last_stream`: wait for it (stream.synchronize() / wait_stream) before
        reading them from another stream."""
        i = self.slot()
        self.k += 1
        st = self.streams[i]
        self.last_stream = st
        self.last_engine = self.engines[i]
        if st is None:
            return fn(self.engines[i])
        st.wait_stream(torch.cuda.current_stream(self.device))
        for t in inputs:
            t.record_stream(st)
        with torch.cuda.stream(st):
            return fn(self.engines[i])

    def predict_graphed(self, x, T, seed=0, cnt0=0, group=None, kind=None, shard=False, always_reduce=False):
        """``engine.predict(x, T, seed, cnt0=cnt0)`` of the next slot as ONE hipGraph launch (torch.cuda.CUDAGraph on ROCm).
        The library neither allocates nor synchronises inside bmi_forward_mcd / bmi_finalize, so the whole batch step — zero
        the moments, the once-per-batch prefix, every sample chunk of the suffix, finalize — is captured once per
        (slot, batch size, T, seed, cnt0) and replayed on the slot's static input buffer; a batch of another size (a loader's
        smaller last batch) is captured on first sight.  What it buys: the small-model configs are launch-bound — VGG-11 at
        batch 250 x T = 30 is 20 launches of 20-50 us on a ~20 us floor each — and a replay issues them back to back.
        Results are bit for bit the eager ones (tests/test_gpu_model.py).

        With a process group of more than one rank (``group``; ``shard=True`` takes the default group of an initialised ``torch.distributed``) the
        graph holds THIS RANK'S SHARE of the step (``sharding.accumulate_share``: its samples, or its images when T < ranks — one
        Masksembles mask of config 4 per GPU is exactly such a launch-bound step) and the all-reduce + finalize follow the replay
        eagerly on the slot's stream: a collective is never captured.

        The scalars of a launch (seed, first sample index, Masksembles counter) are baked into the captured kernel arguments:
        batches that must differ in them get a graph each — keep seed / cnt0 constant over a loader walk, or the cache (at most
        ``graph_cache_max`` graphs per slot, least recently used evicted with its static buffers) turns over.  Engine profiling
        (bmi_profile_enable records events) cannot be captured: refused.  A capture that fails runs the step eagerly instead.
        Returns the slot's STATIC output tensors: read them (after `last_stream`) before the slot comes round again, i.e. within
        the next len(engines) - 1 submissions."""
        from .sharding import _rank_world, accumulate_share
        # a share of the step only when the caller names the group (or shard=True for the default one): a data-parallel caller with a
        # different batch on each rank must not have its ranks' moments summed behind its back
        rank, world = _rank_world(group) if (group is not None or shard) else (0, 1)
        i = self.slot()
        eng = self.engines[i]
        if not hasattr(self, "_graphs"):
            from collections import OrderedDict
            self._graphs = [OrderedDict() for _ in self.engines]
            self._gstreams = [st if st is not None else torch.cuda.Stream(self.device) for st in self.streams]
        key = (tuple(x.shape), int(T), int(seed), int(cnt0), rank, world, kind, bool(always_reduce))
        cache = self._graphs[i]
        rec = cache.get(key)
        if rec is None and eng.profiling:          # (before the slot rotation advances: a refused call leaves the pipe as it was)
            raise RuntimeError("predict_graphed while engine profiling is on: the event records of bmi_profile_enable cannot be captured")
        self.k += 1
        st = self._gstreams[i]
        self.last_stream = st
        self.last_engine = eng
        cur = torch.cuda.current_stream(self.device)

        reduce = world > 1 or bool(always_reduce)        # (always_reduce: the collective in a group of ONE rank too — the 1-GPU RCCL probe)

        def eager():
            st.wait_stream(cur)
            x.record_stream(st)
            with torch.cuda.stream(st):
                S = eng.new_moments(x.shape[0])
                accumulate_share(eng, x, S, T, seed, cnt0, rank, world, kind)
                if reduce:
                    import torch.distributed as dist
                    dist.all_reduce(S, op=dist.ReduceOp.SUM, group=group)
                return eng.finalize(S, T)

        if rec is None:
            xs = torch.empty_like(x)
            S = eng.new_moments(x.shape[0])
            st.wait_stream(cur)
            with torch.cuda.stream(st):                          # warm-up on the capture stream (module load, first launches)
                xs.copy_(x)
                accumulate_share(eng, xs, S, T, seed, cnt0, rank, world, kind)
            st.synchronize()
            graph, out = torch.cuda.CUDAGraph(), {}
            try:
                with torch.cuda.graph(graph, stream=st):
                    S.zero_()
                    accumulate_share(eng, xs, S, T, seed, cnt0, rank, world, kind)
                    if not reduce:
                        out.update(eng.finalize(S, T))
            except Exception as exc:                              # (a launcher returned non-OK under capture, ...)
                import warnings
                warnings.warn(f"hipGraph capture of a batch step failed ({exc}); running eagerly")
                torch.cuda.synchronize(self.device)
                cache[key] = "eager"
                return eager()
            rec = cache[key] = (graph, xs, S, out)
            while len(cache) > self.graph_cache_max:
                cache.popitem(last=False)                          # least recently used: its graph and static buffers are freed
        if rec == "eager":
            return eager()
        cache.move_to_end(key)
        graph, xs, S, out = rec
        st.wait_stream(cur)
        x.record_stream(st)
        with torch.cuda.stream(st):
            xs.copy_(x, non_blocking=True)
            graph.replay()
            if reduce:
                import torch.distributed as dist
                dist.all_reduce(S, op=dist.ReduceOp.SUM, group=group)
                return eng.finalize(S, T)
        return out

    graph_cache_max = 8

    def synchronize(self):
        for st in list(self.streams) + list(getattr(self, "_gstreams", [])):
            if st is not None:
                st.synchronize()

