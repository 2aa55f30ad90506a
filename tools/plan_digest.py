#!/usr/bin/env python3
"""Digest of everything the host-side queries say about a built and planned engine, one line per case: the record an engine refactor
compares against its parent (run it at both commits; the outputs must be identical line for line).  Host only: no GPU, no HIP call.

    python tools/plan_digest.py [--workloads a,b] [--summary] [--out FILE]

Per case, ``CompiledGraph(model, "cpu", max_batch, chunk, dtype)`` and a sha256 over: workspace_bytes; bmi_query's four numbers;
bmi_tensor_info of id = 1, 2, ... until it answers BMI_ERR_INVALID (so the number of tensors is part of it); op_stages(fe) and
exit_stages(fe) of every first_exit.  A combination the engine refuses is printed with its return code.  Then a fixed list of malformed
descriptors and the return code bmi_create gives each.  ``--summary`` folds the switch settings of a (workload, dtype, plan) into one line — their
number, how many were refused, how many distinct digests, and a sha256 over the lines they would have printed — for a record that is kept.

NOT covered, because no host query exposes them: pool_ok / pool_pw_ok / pair_pool_ok, lazy_planar(_plan), the per-op nsplit and out_mul.
tools/engine_identity.py (launch tables and output bits, on a GPU) covers those.
"""
import argparse
import ctypes as C
import hashlib
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402
from bayesnn_fpga_amd import _lib  # noqa: E402
from bayesnn_fpga_amd import engine as engine_mod  # noqa: E402

DTYPES = ("f16", "bf16", "f32", "f16x2", "bf16x3")
PLANS = ((250, 102), (37, 4), (5, 1), (1367, 3))
# process-default switches, one at a time: (name, value, the default it is put back to)
OPTIONS = (("conv_seam", 0, 1), ("pair_prefix", 0, 1), ("splitk", 0, 1), ("splitk_tiles", 0, 64), ("conv_patch64", 0, 1),
           ("conv_s2", 0, 1), ("conv_s2", 2, 1), ("ws_no_reuse", 1, 0), ("mask_lazy", 0, 1))
ENVS = (("BMI_MASK_BITS", "1"), ("BMI_CONV_PAIR", "0"))      # read by getenv at every bmi_create
ERR_INVALID = -22


class Switch:
    """One switch set for the duration of a ``with`` block and put back after it; ``None``: nothing set."""

    def __init__(self, name=None, value=None, default=None):
        self.name, self.value, self.default = name, value, default
        self.label = "default" if name is None else f"{name}={value}"

    def __enter__(self):
        if self.name is None:
            return self
        if self.default is None:
            self.saved = os.environ.get(self.name)
            os.environ[self.name] = self.value
        else:
            _lib.set_option(self.name, self.value)
        return self

    def __exit__(self, *exc):
        if self.name is None:
            return
        if self.default is not None:
            _lib.set_option(self.name, self.default)
        elif self.saved is None:
            del os.environ[self.name]
        else:
            os.environ[self.name] = self.saved


SWITCHES = [Switch()] + [Switch(*o) for o in OPTIONS] + [Switch(n, v) for n, v in ENVS]


def build_seeded(cls, kwargs):
    """The construction of tests/helpers.build_seeded."""
    torch.manual_seed(0)
    np.random.seed(0)
    return cls(**kwargs)


def describe(cg):
    """Everything the host queries return for one planned engine, as one printable structure."""
    query = (cg.prefix_macs, cg.suffix_macs, cg.n_prefix_ops, cg.n_suffix_ops)
    tensors = []
    tid = 1
    while True:
        off = C.c_int64(-1)
        v = [C.c_int32(-1) for _ in range(5)]
        rc = cg.lib.bmi_tensor_info(cg.handle, tid, C.byref(off), *[C.byref(x) for x in v])
        if rc == ERR_INVALID:
            break
        tensors.append((tid, rc, off.value) + tuple(x.value for x in v))
        tid += 1
    stages = [(fe, cg.op_stages(fe), [sorted(d.items()) for d in cg.exit_stages(fe)]) for fe in range(cg.n_exits)]
    return cg.workspace_bytes, query, tensors, stages


def plan_cases(workloads, out, summary=False):
    graphs = {}
    real_build_graph = engine_mod.build_graph

    def cached_build_graph(model, device, dtype="f16"):
        # the graph (ops, folded weights) depends on the model and the dtype only: build it once for all plans and switches of a pair
        key = (id(model), dtype)
        if key not in graphs:
            graphs[key] = real_build_graph(model, device, dtype)
        return graphs[key]

    engine_mod.build_graph = cached_build_graph
    try:
        for name in workloads:
            wl = bench.WORKLOADS[name]
            model = build_seeded(bench._load(wl[0]), wl[2]).eval()
            for dtype in DTYPES:
                for max_batch, chunk in PLANS:
                    lines = []
                    emit = lines.append if summary else out
                    for sw in SWITCHES:
                        label = f"{name}/{dtype} B={max_batch} chunk={chunk} {sw.label}"
                        with sw:
                            try:
                                cg = engine_mod.CompiledGraph(model, "cpu", max_batch, chunk, dtype)
                            except _lib.BmiError as err:
                                emit(f"{label:64s} refused rc={err.code} ({str(err).split(' failed')[0]})")
                                continue
                            ws, query, tensors, stages = describe(cg)
                            cg.close()
                        sha = hashlib.sha256(repr((ws, query, tensors, stages)).encode()).hexdigest()[:32]
                        emit(f"{label:64s} ws={ws} ops={query[2]}+{query[3]} tensors={len(tensors)} sha={sha}")
                    if summary:
                        refused = sum(" refused rc=" in ln for ln in lines)
                        distinct = len({ln.split(" sha=")[1] for ln in lines if " sha=" in ln})
                        sha = hashlib.sha256("\n".join(lines).encode()).hexdigest()[:32]
                        out(f"{name + '/' + dtype:30s} B={max_batch:<4d} chunk={chunk:<3d} settings={len(lines)} refused={refused} distinct={distinct} sha={sha}")
                graphs.clear()
    finally:
        engine_mod.build_graph = real_build_graph


PTR = 0x1000      # a dummy non-null pointer: bmi_create dereferences none


def _op(kind, in_, out, **kw):
    d = _lib.OpDesc()
    d.kind, d.in_, d.out = kind, in_, out
    d.residual, d.in2 = kw.get("residual", -1), kw.get("in2", -1)
    d.ksize, d.stride, d.pad, d.relu = kw.get("ksize", 3), kw.get("stride", 1), kw.get("pad", 1), 1
    d.weight, d.scale, d.bias = PTR, kw.get("scale", PTR), PTR
    d.weight2 = PTR if d.in2 >= 0 else None
    d.site = kw.get("site", _lib.make_site())
    d.site_pos = kw.get("site_pos", _lib.SITE_POS_OUTER)
    d.bias_post = PTR if d.site_pos == _lib.SITE_POS_INNER else None
    return d


def _create(tensors, ops, n_exits=1, out_dim=10, dtype="f16"):
    tarr = (_lib.TensorDesc * len(tensors))(*[_lib.TensorDesc(*t) for t in tensors])
    oarr = (_lib.OpDesc * len(ops))(*ops)
    desc = _lib.ModelDesc(len(tensors), tarr, len(ops), oarr, n_exits, out_dim, _lib.DTYPES[dtype])
    handle = C.c_void_p()
    rc = _lib.lib().bmi_create(C.byref(desc), C.byref(handle))
    if rc == _lib.BMI_OK:
        _lib.lib().bmi_destroy(handle)
    return rc


def malformed_cases(out):
    L = _lib
    stem, conv, head = (lambda o=1, i=0, **k: _op(L.OP_STEM, i, o, **k)), (lambda i, o, **k: _op(L.OP_CONV, i, o, **k)), \
        (lambda i, x=0, **k: _op(L.OP_HEAD, i, x, **k))
    T = [(32, 32, 3), (32, 32, 64), (32, 32, 64), (16, 16, 64), (16, 16, 128), (1, 1, 64)]
    elem = L.make_site(L.SITE_ELEMENTWISE, 0, 0.25)
    chan = L.make_site(L.SITE_CHANNEL, 0, 0.25)
    mask = L.make_site(L.SITE_MASKSEMBLE, 0, 0.0, 4, PTR)
    down = dict(ksize=3, stride=2, pad=1)
    cases = [
        ("well-formed (stem, conv, head)", dict(tensors=T, ops=[stem(), conv(1, 2), head(2)])),
        ("an output tensor written twice", dict(tensors=T, ops=[stem(), conv(1, 2), conv(1, 2), head(2)])),
        ("an input never written", dict(tensors=T, ops=[stem(), conv(3, 2), head(2)])),
        ("an exit without a head", dict(tensors=T, ops=[stem(), conv(1, 2), head(2)], n_exits=2)),
        ("a head index used twice", dict(tensors=T, ops=[stem(), conv(1, 2), head(2), head(1)], n_exits=2)),
        ("a STEM not on tensor 0", dict(tensors=T, ops=[stem(), stem(2, 1), head(2)])),
        ("a CONV on tensor 0", dict(tensors=T, ops=[conv(0, 1), conv(1, 2), head(2)])),
        ("a residual of another shape", dict(tensors=T, ops=[stem(), conv(1, 3, **down), conv(1, 2, residual=3), head(2)])),
        ("Cin % 64 != 0 on an f16 engine", dict(tensors=[(32, 32, 3), (32, 32, 32), (32, 32, 64)], ops=[stem(), conv(1, 2), head(2)])),
        ("out_dim = 129", dict(tensors=T, ops=[stem(), conv(1, 2), head(2)], out_dim=129)),
        ("an inner site on a conv with a shortcut input",
         dict(tensors=T, ops=[stem(), conv(1, 3, **down), conv(3, 4, in2=1, scale=None, site=elem, site_pos=L.SITE_POS_INNER), head(4)])),
        ("a Masksembles inner site", dict(tensors=T, ops=[stem(), conv(1, 2, site=mask, site_pos=L.SITE_POS_INNER), head(2)])),
        ("a DENSE on a non-1x1 map", dict(tensors=T, ops=[stem(), _op(L.OP_DENSE, 1, 5), head(5)])),
        ("an inner non-elementwise site on a head", dict(tensors=T, ops=[stem(), conv(1, 2), head(2, site=chan, site_pos=L.SITE_POS_INNER)])),
    ]
    for label, kw in cases:
        out(f"malformed: {label:48s} bmi_create rc={_create(**kw)}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workloads", default=",".join(bench.WORKLOADS), help="comma-separated names of bench.py's WORKLOADS (default: all)")
    ap.add_argument("--summary", action="store_true", help="one line per (workload, dtype, plan) over its switch settings")
    ap.add_argument("--out", default="", help="also write the lines to this file")
    a = ap.parse_args()
    f = open(a.out, "w") if a.out else None

    def out(line):
        print(line, flush=True)
        if f:
            f.write(line + "\n")

    plan_cases([w for w in a.workloads.split(",") if w], out, a.summary)
    malformed_cases(out)
    if f:
        f.close()


if __name__ == "__main__":
    main()
