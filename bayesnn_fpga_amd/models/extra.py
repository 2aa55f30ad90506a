"""Build-defined models for the BASELINE configs that have NO PyTorch counterpart in the reference
(SURVEY.md §8.0): VGG-11-BN with dropout before its dense layers (config 2) and a multi-exit ResNet-50
(config 5).  Architectures are taken from the reference's Keras definitions / its ``Bottleneck`` block:

* ``VGG11MC``             — Hardware_Artifact/bayes_hw/models/models.py:211-287 (64 filters, dense 512/512/C; the
  ``num_bayes_layer`` counter rule over its 7 candidate sites; 3 = dropout before each dense layer).
* ``ResNet50MCEarlyExit`` — SA/models/resnet18/resnet18.py:51-85 (Bottleneck), :88-180 with [3,4,6,3]; the first conv
  of every exit head takes the stage's real width (the reference's 64/128/256-channel heads make the
  Bottleneck network fail in ``ex1conv1``).
Parity for these is pinned against the fp32 CPU restatement in ``oracle/extra_models.py`` only.  Dense layers run
as 1x1 convolutions on [N,1,1,C] tensors (same MFMA kernel, same fused dropout epilogue).
* ``LeNet5MC``            — config 1, Hardware_Artifact/bayes_hw/models/models.py:34-73 (``lenet``; the counter rule over its 3 candidate
  sites).  Its 5x5 convs on 1 and 20 channels, 7x7 pool and 80 -> 100 -> C dense layers lie outside the graph engine's kernels: it runs
  as ONE fused kernel per call (csrc/lenet5.hip) behind ``engine.LeNet5Engine``, not through ``MCDEngine``.
* ``LeNet5MCEarlyExit``   — the multi-exit form of that LeNet, Hardware_Artifact/bayes_hw/models/t_qmodels_bayes_me.py:41-147
  (``T_Qlenet_bayes_me``): an early exit on the pooled conv1 map and one MC-dropout layer in front of each exit's classifier; ONE fused
  kernel per call as well (csrc/lenet5_me.hip), behind the same ``engine.LeNet5Engine``; with ``quant_tbit`` the QKeras model itself, in
  fixed point (csrc/qlenet5_me.hip).
"""
import math

from torch import nn

from ..utils import Masksembles1D, Masksembles2D
from ._engine_mixin import EngineModelMixin
from .resnet18.resnet18 import MCDropout, _no_cpu

VGG11_CFG = (64, 'M', 128, 'M', 256, 256, 'M', 512, 512, 'M', 512, 512, 'M')


def _he_init(model):
    for m in model.modules():
        if isinstance(m, nn.Conv2d):
            m.weight.data.normal_(0, math.sqrt(2.0 / (m.kernel_size[0] * m.kernel_size[1] * m.out_channels)))
        elif isinstance(m, nn.BatchNorm2d):
            m.weight.data.fill_(1)
            m.bias.data.zero_()


class VGG11MC(EngineModelMixin, nn.Module):
    family = "vgg11"
    multi_exit = False

    def __init__(self, num_bayes_layer=3, dropout_p=0.25, out_dim=10, dense=(512, 512)):
        super().__init__()
        self.n_exits, self.out_dim, self.dropout_p, self.num_bayes_layer = 1, out_dim, dropout_p, num_bayes_layer
        first_site = 7 - num_bayes_layer
        feats, cin, loc = [], 3, 0
        for v in VGG11_CFG:
            if v == 'M':
                feats.append(nn.MaxPool2d(2, 2))
                if loc < 4:
                    if loc >= first_site:
                        feats.append(MCDropout(dropout_p))
                    loc += 1
            else:
                feats += [nn.Conv2d(cin, v, 3, padding=1), nn.BatchNorm2d(v), nn.ReLU(inplace=True)]
                cin = v
        self.features = nn.Sequential(*feats)
        cls, cin = [], 512
        if 4 >= first_site:
            cls.append(MCDropout(dropout_p))
        for i, d in enumerate(dense):
            cls += [nn.Linear(cin, d), nn.ReLU(inplace=True)]
            if 5 + i >= first_site:
                cls.append(MCDropout(dropout_p))
            cin = d
        cls.append(nn.Linear(cin, out_dim))
        self.classifier = nn.Sequential(*cls)
        _he_init(self)
        self._init_engine_state()

    def build_graph(self, g):
        x = g.tensor(32, 32, 3)
        mods, i, first = list(self.features), 0, True
        while i < len(mods):
            m = mods[i]
            if isinstance(m, nn.Conv2d):
                x = g.conv(x, m, mods[i + 1], relu=True, stem=first)
                first = False
                i += 3
            elif isinstance(m, nn.MaxPool2d):
                x = g.maxpool(x)
                i += 1
            elif isinstance(m, nn.Dropout):
                x = g.mask(x, g.site(m))
                i += 1
            else:
                raise TypeError(type(m).__name__)
        cls, i = list(self.classifier), 0
        pending = None                        # a site that precedes the next dense layer
        while i < len(cls):
            m = cls[i]
            if isinstance(m, nn.Dropout):
                pending = m
                i += 1
            elif isinstance(m, nn.Linear) and i + 1 < len(cls):       # hidden dense + ReLU (+ dropout)
                if pending is not None:
                    x = g.mask(x, g.site(pending))
                    pending = None
                nxt = cls[i + 2] if i + 2 < len(cls) and isinstance(cls[i + 2], nn.Dropout) else None
                x = g.dense(x, m, relu=True, site=g.site(nxt))
                i += 3 if nxt is not None else 2
            else:                                                       # final classifier
                g.head(x, m, 0, site=g.site(pending))
                i += 1


class LeNet5MC(EngineModelMixin, nn.Module):
    """MC-dropout LeNet-5 on 28x28x1 inputs.  Candidate sites A (behind the first pool), B (behind flatten), C (behind fc1 + ReLU);
    ``num_bayes_layer = k`` switches on the last k (models.py:36-68 with num_layers = 3); k = 1 is the oracle's ``LeNet5MC``.  Sites are
    elementwise, numbered 0, 1, ... in call order over those that are on.  ``mask_type="mask"`` (the hardware flow's ``dropout_type``,
    model_utils.py:43-52) puts ``Masksembles2D(20)`` / ``Masksembles1D(80)`` / ``Masksembles1D(100)`` of ``num_masks`` masks in their places:
    csrc/lenet5_mask.hip.  ``quant_tbit = W`` (with ``quant_ibit = I``) makes it the hardware flow's QKeras model ``T_Qlenet_bayes``
    (t_qmodels_bayes.py:38-96): the same fp32 parameters, quantised to W-bit codes when the engine is built (``quant.weight_codes``) and run in
    fixed point by csrc/qlenet5.hip; MC dropout only."""
    family = "lenet5"
    multi_exit = False
    engine_dtype = "f16"

    def __init__(self, num_bayes_layer=1, dropout_p=0.2, out_dim=10, mask_type="mc", num_masks=4, mask_scale=2.0, quant_tbit=None, quant_ibit=0):
        super().__init__()
        if num_bayes_layer not in (0, 1, 2, 3):
            raise ValueError("num_bayes_layer must be 0, 1, 2 or 3")
        if mask_type not in ("mc", "mask"):
            raise ValueError("mask_type must be 'mc' or 'mask'")
        if quant_tbit is not None:
            if mask_type != "mc":
                raise ValueError("the quantised LeNet-5 takes MC-dropout sites only: quant_tbit needs mask_type='mc'")
            if not (isinstance(quant_tbit, int) and isinstance(quant_ibit, int) and 2 <= quant_tbit <= 8 and 0 <= quant_ibit < quant_tbit):
                raise ValueError("quant_tbit must be an int in [2, 8] and quant_ibit one in [0, quant_tbit - 1]")
        self.quant_tbit, self.quant_ibit = quant_tbit, quant_ibit
        self.n_exits, self.out_dim, self.dropout_p, self.num_bayes_layer = 1, out_dim, dropout_p, num_bayes_layer
        self.mask_type, self.num_masks, self.mask_scale = mask_type, num_masks, mask_scale
        self.conv1 = nn.Conv2d(1, 20, 5, padding=2)
        self.conv2 = nn.Conv2d(20, 20, 5, padding=2)
        self.fc1 = nn.Linear(80, 100)
        for loc, (name, cls, channels) in enumerate((("drop_a", Masksembles2D, 20), ("drop_b", Masksembles1D, 80), ("drop", Masksembles1D, 100))):
            if loc >= 3 - num_bayes_layer:      # ("drop": the oracle's name for site C)
                setattr(self, name, MCDropout(dropout_p) if mask_type == "mc" else cls(channels, num_masks, mask_scale))
        self.fc2 = nn.Linear(100, out_dim)
        self._init_engine_state()

    def site_mods(self):
        """The modules of sites A, B, C (None: off)."""
        return [getattr(self, name, None) for name in ("drop_a", "drop_b", "drop")]

    def site_descs(self, mask_ptrs=None):
        """The three ``_lib.Site`` of bmi_lenet5_desc, A, B, C: off, elementwise with the module's p and its call-order id, or Masksembles
        with the module's n and ``mask_ptrs[i]``, the device address of its masks as fp32 [n][channels] (None: a null pointer)."""
        from .. import _lib
        ids = iter(range(3))
        return [_lib.make_site() if m is None else
                _lib.make_site(_lib.SITE_ELEMENTWISE, next(ids), m.p) if isinstance(m, MCDropout) else
                _lib.make_site(_lib.SITE_MASKSEMBLE, next(ids), 0.0, m.n, mask_ptrs[i] if mask_ptrs else None)
                for i, m in enumerate(self.site_mods())]

    def engine(self, device, max_batch=None, **_):
        """The compiled ``engine.LeNet5Engine`` for ``device`` (built on first use, rebuilt when it must grow)."""
        from ..engine import LeNet5Engine
        key, need = str(device), max_batch or 1
        eng = self._engines.get(key)
        if eng is None or eng.max_batch < need:
            if eng is not None:
                eng.close()
            eng = self._engines[key] = LeNet5Engine(self, device, max_batch=max(need, eng.max_batch if eng else 0))
        return eng


class LeNet5MCEarlyExit(EngineModelMixin, nn.Module):
    """Multi-exit MC-dropout LeNet-5 on 28x28x1 inputs: ``LeNet5MC``'s trunk under the same parameter names plus an early exit on the
    pooled conv1 map [B, 20, 14, 14] — conv 5x5x20 with stride 7 (Keras "same" at stride 7 on a 14-wide map pads nothing: outputs 2x2),
    ReLU, flatten, Linear 80 -> 100, ReLU, Linear 100 -> C.  ``dropout_exit`` puts one elementwise MC-dropout layer on the 100 hidden units
    in front of each exit's classifier.  Exits in depth order: exit 0 is the early exit, exit 1 (the last) the main exit; site ids follow
    that call order.  ``quant_tbit = W`` (with ``quant_ibit = I``) makes it the QKeras model ``T_Qlenet_bayes_me`` itself
    (t_qmodels_bayes_me.py:41-147): the same modules and fp32 parameters, quantised to W-bit codes when the engine is built
    (``quant.weight_codes``) and run in fixed point by csrc/qlenet5_me.hip."""
    family = "lenet5_me"
    multi_exit = True
    engine_dtype = "f16"

    def __init__(self, dropout_exit=True, dropout_p=0.2, out_dim=10, quant_tbit=None, quant_ibit=0):
        super().__init__()
        if quant_tbit is not None and not (isinstance(quant_tbit, int) and isinstance(quant_ibit, int) and 2 <= quant_tbit <= 8 and 0 <= quant_ibit < quant_tbit):
            raise ValueError("quant_tbit must be an int in [2, 8] and quant_ibit one in [0, quant_tbit - 1]")
        self.quant_tbit, self.quant_ibit = quant_tbit, quant_ibit
        self.n_exits, self.out_dim, self.dropout_p, self.dropout_exit = 2, out_dim, dropout_p, dropout_exit
        self.conv1 = nn.Conv2d(1, 20, 5, padding=2)
        self.conv2 = nn.Conv2d(20, 20, 5, padding=2)
        self.fc1 = nn.Linear(80, 100)
        self.fc2 = nn.Linear(100, out_dim)
        self.ex1conv1 = nn.Conv2d(20, 20, 5, stride=7, padding=0)
        self.ex1fc1 = nn.Linear(80, 100)
        self.ex1linear = nn.Linear(100, out_dim)
        if dropout_exit:
            self.exit1_dropout = MCDropout(dropout_p)
            self.exit_dropout = MCDropout(dropout_p)
        self._init_engine_state()

    def site_descs(self):
        """The two ``_lib.Site`` of bmi_lenet5_me_desc, early exit then main exit: off, or elementwise with the module's p and its call-order id."""
        from .. import _lib
        mods = [getattr(self, name, None) for name in ("exit1_dropout", "exit_dropout")]
        return [_lib.make_site() if m is None else _lib.make_site(_lib.SITE_ELEMENTWISE, i, m.p) for i, m in enumerate(mods)]

    engine = LeNet5MC.engine


class Bottleneck(nn.Module):
    expansion = 4

    def __init__(self, inplanes, planes, stride=1, downsample=None):
        super().__init__()
        self.planes = planes
        self.conv1 = nn.Conv2d(inplanes, planes, 1, bias=False)
        self.bn1 = nn.BatchNorm2d(planes)
        self.conv2 = nn.Conv2d(planes, planes, 3, stride=stride, padding=1, bias=False)
        self.bn2 = nn.BatchNorm2d(planes)
        self.conv3 = nn.Conv2d(planes, planes * 4, 1, bias=False)
        self.bn3 = nn.BatchNorm2d(planes * 4)
        self.downsample = downsample
        self.stride = stride

    forward = _no_cpu


class ResNet50MCEarlyExit(EngineModelMixin, nn.Module):
    family = "resnet50"
    multi_exit = True

    def __init__(self, dropout_exit=True, dropout="block", dropout_p=0.25, out_dim=10, num_blocks=(3, 4, 6, 3)):
        super().__init__()
        self.n_exits, self.out_dim = 4, out_dim
        self.dropout_exit, self.dropout, self.dropout_p, self.mask_type = dropout_exit, dropout, dropout_p, "mc"
        self.inplanes = 64
        self.conv1 = nn.Conv2d(3, 64, 3, 1, 1, bias=False)
        self.bn1 = nn.BatchNorm2d(64)
        for i, (planes, stride) in enumerate(((64, 1), (128, 2), (256, 2), (512, 2)), 1):
            setattr(self, f"layer{i}", self._make_layer(planes, num_blocks[i - 1], stride))
        self.linear = nn.Linear(2048, out_dim)
        for e, chans in ((1, (256, 128, 256, 512)), (2, (512, 256, 512)), (3, (1024, 512))):
            for j, (a, b) in enumerate(zip(chans[:-1], chans[1:]), 1):
                setattr(self, f"ex{e}conv{j}", nn.Conv2d(a, b, 3, 2, 1, bias=False))
                setattr(self, f"ex{e}bn{j}", nn.BatchNorm2d(b))
            setattr(self, f"ex{e}linear", nn.Linear(512, out_dim))
        _he_init(self)
        if dropout == "block":
            for i in (1, 2, 3):
                setattr(self, f"layer{i}", nn.Sequential(getattr(self, f"layer{i}"), MCDropout(dropout_p)))
        elif dropout is not None:
            raise ValueError("only dropout in {None, 'block'} is defined for the ResNet-50 config")
        if dropout_exit:
            for name in ("exit1_dropout", "exit2_dropout", "exit3_dropout", "exit_dropout"):
                setattr(self, name, MCDropout(dropout_p))
        self._init_engine_state()

    def _make_layer(self, planes, blocks, stride):
        down = None
        if stride != 1 or self.inplanes != planes * 4:
            down = nn.Sequential(nn.Conv2d(self.inplanes, planes * 4, 1, stride, bias=False), nn.BatchNorm2d(planes * 4))
        layers = [Bottleneck(self.inplanes, planes, stride, down)]
        self.inplanes = planes * 4
        layers += [Bottleneck(self.inplanes, planes) for _ in range(1, blocks)]
        return nn.Sequential(*layers)

    def build_graph(self, g):
        from ..engine import _unwrap
        x = g.tensor(32, 32, 3)
        x = g.conv(x, self.conv1, self.bn1, relu=False, stem=True)
        for si in range(1, 5):
            stage, stage_site = _unwrap(getattr(self, f"layer{si}"))
            blocks = list(stage)
            for bi, blk in enumerate(blocks):
                site_mod = stage_site if bi == len(blocks) - 1 else None
                a = g.conv(x, blk.conv1, blk.bn1, relu=True)
                b = g.conv(a, blk.conv2, blk.bn2, relu=True)
                res = x if blk.downsample is None else g.conv(x, blk.downsample[0], blk.downsample[1], relu=False)
                x = g.conv(b, blk.conv3, blk.bn3, relu=True, residual=res, site=g.site(site_mod))
            if si < 4:
                y = x
                for j in range(1, 5 - si):
                    y = g.conv(y, getattr(self, f"ex{si}conv{j}"), getattr(self, f"ex{si}bn{j}"), relu=True)
                sm = getattr(self, f"exit{si}_dropout", None) if self.dropout_exit else None
                g.head(y, getattr(self, f"ex{si}linear"), si - 1, site=g.site(sm))
        sm = getattr(self, "exit_dropout", None) if self.dropout_exit else None
        g.head(x, self.linear, 3, site=g.site(sm))
