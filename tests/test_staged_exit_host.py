"""CPU-side checks of early exit by stages (bmi_forward_mcd_exit_staged, bmi_query_exit_stages, MCDEngine.predict_early_exit): every
bad argument gets its return code before any launch, and the stage plan of the exit-only models puts each op at the smallest exit index
downstream of it.  The graphs live on the CPU, so a call that got as far as a launch would fail with a HIP error instead."""
import ctypes as C

import numpy as np
import pytest
import torch.nn as nn

from bayesnn_fpga_amd import _lib
from bayesnn_fpga_amd.engine import CompiledGraph
from bayesnn_fpga_amd.models.resnet18.resnet18 import ResNet18MCEarlyExit
from bayesnn_fpga_amd.models.vgg19.vgg19 import VGG19MCEarlyExit
from tests.helpers import build_seeded

KW = dict(dropout_exit=True, dropout="block", dropout_p=0.25, out_dim=10)
EXIT_ONLY = dict(dropout_exit=True, dropout=None, dropout_p=0.25, out_dim=100)


def _graph(cls=ResNet18MCEarlyExit, kw=KW, dtype="f16", max_batch=8, chunk=4):
    return CompiledGraph(build_seeded(cls, kw), "cpu", max_batch, chunk, dtype=dtype)


def test_staged_entry_point_checks_arguments_before_any_launch():
    cg = _graph()
    lib, h, ws_ok, E = _lib.lib(), cg.handle, cg.workspace_bytes, cg.n_exits
    buf = np.zeros(64, dtype=np.float64)                  # a non-null address; no row gets far enough to use it
    p = buf.ctypes.data
    act = (C.c_int32 * 64)()

    def st(h=h, x=p, batch=8, t=4, cnt0=0, crit=0, ens=0, thr=0.5, fe=1, rule=True, S1=p, S2=p, SL=p, SH=p, xo=p, act=act, ws=p, nbytes=ws_ok):
        r = _lib.ExitRule(crit, ens, thr, fe)
        return lib.bmi_forward_mcd_exit_staged(h, x, batch, t, 7, cnt0, C.byref(r) if rule else None, S1, S2, SL, SH, xo, act, ws, nbytes, None)

    small = ws_ok - 1
    rows = [
        (st(h=None), -22), (st(x=None), -22), (st(rule=False), -22), (st(S1=None), -22), (st(S2=None), -22), (st(SL=None), -22),
        (st(xo=None), -22), (st(act=None), -22), (st(ws=None), -22),
        (st(crit=2), -22), (st(crit=-1), -22), (st(ens=2), -22), (st(ens=-1), -22), (st(thr=float("nan")), -22),
        (st(fe=-1), -22), (st(fe=E), -22), (st(batch=0), -22), (st(batch=9), -22), (st(t=0), -22), (st(cnt0=-1), -22),
        (st(crit=7, t=5), -22), (st(fe=E, nbytes=small), -22), (st(batch=9, nbytes=small), -22),
        (st(t=5), -95), (st(t=5, nbytes=small), -95), (st(nbytes=small), -12),
        (st(SH=None, nbytes=small), -12),                    # SH is optional
        (st(crit=1, ens=1, fe=0, nbytes=small), -12), (st(fe=E - 1, thr=float("inf"), nbytes=small), -12),
    ]
    assert [rc for rc, _ in rows] == [want for _, want in rows]


def test_staged_exit_refuses_the_exact_engine():
    cg = _graph(dtype="f32")
    lib = _lib.lib()
    buf = np.zeros(64, dtype=np.float64)
    p = buf.ctypes.data
    act = (C.c_int32 * 8)()
    r = _lib.ExitRule(0, 0, 0.5, 1)
    for nbytes in (cg.workspace_bytes, cg.workspace_bytes - 1):
        assert lib.bmi_forward_mcd_exit_staged(cg.handle, p, 8, 4, 7, 0, C.byref(r), p, p, p, None, p, act, p, nbytes, None) == -95


def test_query_exit_stages_checks_arguments():
    cg = _graph()
    lib, E = _lib.lib(), cg.n_exits
    n = C.c_int32(-1)
    arr = (C.c_int64 * 8)()
    assert lib.bmi_query_exit_stages(None, 1, 0, C.byref(n), None, None, None, None, None) == -22
    assert lib.bmi_query_exit_stages(cg.handle, 1, 0, None, None, None, None, None, None) == -22
    assert lib.bmi_query_exit_stages(cg.handle, -1, 0, C.byref(n), None, None, None, None, None) == -22
    assert lib.bmi_query_exit_stages(cg.handle, E, 0, C.byref(n), None, None, None, None, None) == -22
    assert lib.bmi_query_exit_stages(cg.handle, 1, -1, C.byref(n), None, None, None, None, None) == -22
    assert lib.bmi_query_exit_stages(cg.handle, 1, 0, C.byref(n), None, None, None, None, None) == 0 and n.value == E - 1
    assert lib.bmi_query_exit_stages(cg.handle, 1, E - 2, C.byref(n), arr, None, None, None, None) == -22     # too small
    with pytest.raises(ValueError):
        cg.exit_stages(E)


def test_predict_early_exit_rejects_bad_python_arguments():
    """ValueError before the C call (the engine object is built without a GPU: only the checks run)."""
    import torch
    from bayesnn_fpga_amd.engine import MCDEngine

    class Fake(MCDEngine):
        def __init__(self):            # no workspace, no device: the argument checks come first
            self.n_exits, self.chunk_samples, self.max_batch, self.out_dim, self.device = 4, 4, 8, 10, torch.device("cpu")

        def _check_x(self, x):
            return x

    e = Fake()
    x = torch.zeros(2, 3, 32, 32)
    for kw in (dict(rule="entropy"), dict(rule="sem"), dict(T=5), dict(T=0)):
        args = dict(T=4, threshold=0.5)
        args.update(kw)
        with pytest.raises(ValueError):
            e.predict_early_exit(x, **args)
    S = np.zeros(1)
    for kw in (dict(rule="max"), dict(T=5), dict(first_exit=4), dict(first_exit=-1)):
        args = dict(T=4, threshold=0.5)
        args.update(kw)
        with pytest.raises(ValueError):
            e.accumulate_early_exit(x, S, **args)


def _conv_macs(module, hw):
    """MACs per image of the Conv2d layers of ``module`` whose output map is hw x hw."""
    return sum(hw * hw * c.out_channels * c.in_channels * c.kernel_size[0] * c.kernel_size[1] // c.groups
               for c in module.modules() if isinstance(c, nn.Conv2d))


def _check_plan(cg, first_exit):
    st = cg.exit_stages(first_exit)
    E = cg.n_exits
    assert len(st) == E - first_exit
    assert sum(s["prefix_macs"] for s in st) == cg.prefix_macs
    assert sum(s["suffix_macs"] for s in st) == cg.suffix_macs
    assert sum(s["n_ops"] for s in st) == cg.n_prefix_ops + cg.n_suffix_ops
    assert st[0]["whole_batch_macs"] == 0 and st[0]["n_whole_batch_ops"] == 0
    for s in st:
        assert 0 <= s["whole_batch_macs"] <= s["prefix_macs"] and s["n_whole_batch_ops"] <= s["n_ops"]
    # exit-only dropout: the suffix is the heads alone; stage 0 holds heads 0..first_exit, every later stage one head
    head = cg.out_dim * 512
    assert st[0]["suffix_macs"] == (first_exit + 1) * head
    assert all(s["suffix_macs"] == head for s in st[1:])
    return st


@pytest.mark.parametrize("dt", ["f16", "f16x2"])
@pytest.mark.parametrize("B", [45, 250])
def test_stage_plan_of_exit_only_resnet18(dt, B):
    m = build_seeded(ResNet18MCEarlyExit, EXIT_ONLY)
    cg = CompiledGraph(m, "cpu", B, 10, dtype=dt)
    assert cg.suffix_macs == 4 * 512 * 100                      # exit-only: every conv is in the prefix
    st = _check_plan(cg, 1)
    # the last stage is layer4 (4x4 maps) and the final head; stage 0 holds the stem, layer1, layer2, exit 0 / 1 and the layer3 conv
    # paired with an exit-1 branch conv (same input, one launch), so stage 1 holds layer3 and exit 2 without it
    assert st[2]["prefix_macs"] == _conv_macs(m.layer4, 4)
    trunk = cg.prefix_macs
    assert st[1]["prefix_macs"] + st[2]["prefix_macs"] >= 0.4 * trunk      # what an image that leaves at exit 1 never runs
    # first_exit 0 splits stage 0 at exit 0; first_exit E-1 is one stage: the full run
    st0 = _check_plan(cg, 0)
    assert st0[0]["prefix_macs"] + st0[1]["prefix_macs"] == st[0]["prefix_macs"] and st0[2:] == st[1:]
    assert _check_plan(cg, 3)[0]["prefix_macs"] == trunk


def _restated_stages(cg):
    """{tensor id (heads: -1 - exit): stage} from the Python graph: the smallest exit index downstream, transitively (no fusion)."""
    E = cg.n_exits
    tmin = {}
    out = {}
    for o in reversed(cg.graph.ops):
        key = -1 - o["out"] if o["kind"] == _lib.OP_HEAD else o["out"]
        st = o["out"] if o["kind"] == _lib.OP_HEAD else tmin.get(o["out"], E - 1)
        out[key] = st
        for t in (o["in_"], o.get("residual", -1), o.get("in2", -1)):
            if t is not None and t >= 0:
                tmin[t] = min(tmin.get(t, E - 1), st)
    return out


def _check_op_stages(cg, first_exit):
    """Every op's stage is the restated one, folded at first_exit; the two members of a pair-fused op (consecutive entries of the same
    engine op) share the smaller of their two stages.  No op is whole-batch on these models: every prefix kernel has a row-table form."""
    want = {k: max(0, v - first_exit) for k, v in _restated_stages(cg).items()}
    got = cg.op_stages(first_exit)
    assert sorted(o for o, _, _ in got) == sorted(want)
    moved = 0
    for out, st, wb in got:
        assert not wb
        if st != want[out]:
            assert st < want[out]          # only a fused partner moves, and only to an earlier stage
            moved += 1
    return got, moved


@pytest.mark.parametrize("dt", ["f16", "f16x2"])
@pytest.mark.parametrize("B", [45, 250])
def test_op_stages_of_exit_only_resnet18(dt, B):
    """The issue's membership: stem, layer1, layer2 and the exit-0 / exit-1 branches in stage 0; layer3 and exit 2 in stage 1, except a
    layer3 conv pair-fused with an exit-1 branch conv (stage 0); layer4 and the final head in stage 2."""
    cg = CompiledGraph(build_seeded(ResNet18MCEarlyExit, EXIT_ONLY), "cpu", B, 10, dtype=dt)
    for fe in range(cg.n_exits):
        _, moved = _check_op_stages(cg, fe)
    _, moved = _check_op_stages(cg, 1)
    st = cg.exit_stages(1)
    assert all(s["whole_batch_macs"] == 0 for s in st)
    if dt == "f16":
        assert moved == 1              # the layer3 / exit-1 pair (the split engines do not pair prefix convs)
    assert cg.op_stages(1).count((-1 - 3, 2, False)) == 1 and cg.op_stages(1).count((-1 - 1, 0, False)) == 1


@pytest.mark.parametrize("dt", ["f16", "bf16x3"])
@pytest.mark.parametrize("B", [45, 250])
def test_op_stages_of_vgg19_exit_only(dt, B):
    cg = _graph(VGG19MCEarlyExit, EXIT_ONLY, dt, B, 10)
    for fe in range(cg.n_exits):
        _check_op_stages(cg, fe)
    assert all(s["whole_batch_macs"] == 0 for s in cg.exit_stages(1))


@pytest.mark.parametrize("dt", ["f16", "bf16x3"])
def test_stage_plan_of_vgg19_exit_only(dt):
    cg = _graph(VGG19MCEarlyExit, EXIT_ONLY, dt, 250, 10)
    assert cg.n_exits == 5 and cg.suffix_macs == 5 * 512 * 100
    st = _check_plan(cg, 1)
    assert all(s["prefix_macs"] > 0 for s in st)
    for fe in range(cg.n_exits):
        _check_plan(cg, fe)


def test_stage_plan_of_a_stochastic_trunk():
    """Block + exit dropout: the trunk after the stem is per sample; its stages split the suffix, the prefix stays in stage 0."""
    cg = _graph(max_batch=45, chunk=6)
    st = cg.exit_stages(1)
    assert st[0]["prefix_macs"] == cg.prefix_macs and all(s["prefix_macs"] == 0 for s in st[1:])
    assert sum(s["suffix_macs"] for s in st) == cg.suffix_macs and all(s["suffix_macs"] > 0 for s in st)
