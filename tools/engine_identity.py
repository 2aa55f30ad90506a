#!/usr/bin/env python3
"""Same launches, same bits: what an engine refactor runs on one MI355X, once in a tree exported from its parent and once in the new tree
(one process per tree); the lines of the two runs must be identical.  One line per case:

    launches = rows of profile_launches() after the call
    table    = sha256 (32 hex digits) of that table restricted to (kind, family, out, images)
    out      = sha256 (32 hex digits) of dtype, shape and raw bytes of every tensor the call returned, and of the host lists it returned

    python tools/engine_identity.py [--out FILE]

Cases.  Inputs synthetic_images(B, seed=1234), weights synthetic_weights_(model, 0), seed 42.
  1. planned as bench.py plans a workload (max_batch 250, the default chunk): predict at T = 207 (two full chunks and a partial one) on
     the workloads and dtypes of PREDICT; the option variants of VARIANTS; forward_samples with mask_stride = 3; predict_ensemble (plain,
     under a temperature, under a vector scaling with ensemble weights); the dynamic-exit and adaptive families of DYNAMIC.
  2. predict at the small plan max_batch = 37, chunk = 4, T = 9 (SMALL): no planar lazy layout, other split-K counts.
  3. resnet18_me f16 under BMI_MASK_BITS=1 and under BMI_CONV_PAIR=0 (read at bmi_create).
  4. the calibration maps (``calibration_family``; ``--only calibration`` runs nothing else), resnet18_me f16 at max_batch = 37, chunk = 4,
     T = 9: predict_ensemble under a matrix scaling; predict_votes under each of the three maps, with and without ensemble weights;
     ensemble_moments and vote_counts on held forward_samples logits with each map passed as arguments; nll_grid, nll_vector_grad,
     nll_matrix_grad and ensemble_nll_grid on those logits.
The thresholds of the dynamic cases come from the engine's own predictions by the rules of ``exit_threshold`` / ``sem_threshold`` below, so
that images leave at the first tested exit and others go on, and so that the adaptive walk runs its full-grid form first and its image-list
form afterwards; they are printed with each line, as are active_after / active_after_step.
"""
import argparse
import hashlib
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402
from bayesnn_fpga_amd import _lib  # noqa: E402
from bayesnn_fpga_amd.engine import MCDEngine  # noqa: E402
from bayesnn_fpga_amd.synthetic import synthetic_images, synthetic_weights_  # noqa: E402

SEED = 42
PREDICT = (("resnet18_exit_only", "f16"), ("resnet18_layer", "f16"), ("resnet18_masksembles", "f16"), ("resnet18_me", "f16"),
           ("resnet18_me", "bf16"), ("resnet18_me", "f16x2"), ("resnet18_me", "bf16x3"), ("resnet18_me", "f32"), ("resnet50_me", "f16"),
           ("vgg11", "f16"), ("vgg19_me", "f16"))
# (workload, option, value, the default it is put back to): process defaults, set before the engine is created
VARIANTS = (("resnet18_me", "conv_pool", 0, 1), ("resnet18_me", "conv_pool", 1, 1), ("resnet18_me", "conv_pool", 2, 1),
            ("resnet18_me", "mask_lazy", 0, 1), ("resnet50_me", "conv_seam", 0, 1), ("resnet18_me", "splitk", 0, 1))
DYNAMIC = (("resnet18_me", "f16"), ("resnet18_me", "f16x2"), ("resnet18_exit_only", "f16"), ("vgg19_me", "f16"))
SMALL = (("resnet18_me", "f16"), ("resnet18_me", "f16x2"), ("resnet50_me", "f16"), ("vgg19_me", "f16"))
ENVS = (("BMI_MASK_BITS", "1"), ("BMI_CONV_PAIR", "0"))
T_PREDICT, T_ENSEMBLE, T_EXIT, T_MAX, T_STEP = 207, 105, 8, 16, 4

_models = {}


def model_of(name):
    if name not in _models:
        wl = bench.WORKLOADS[name]
        torch.manual_seed(0)
        np.random.seed(0)
        _models[name] = synthetic_weights_(bench._load(wl[0])(**wl[2]), 0).eval()
    return _models[name]


def digest(value):
    """sha256 over a call's result: tensors by dtype, shape and raw bytes, dicts by sorted key, host values by repr."""
    h = hashlib.sha256()

    def add(v):
        if isinstance(v, torch.Tensor):
            a = v.detach().cpu().contiguous()
            h.update(f"{a.dtype}{tuple(a.shape)}".encode())
            h.update(a.view(torch.uint8).numpy().tobytes() if a.numel() else b"")
        elif isinstance(v, dict):
            for k in sorted(v):
                h.update(str(k).encode())
                add(v[k])
        elif isinstance(v, (list, tuple)) and any(isinstance(x, (torch.Tensor, dict)) for x in v):
            for x in v:
                add(x)
        else:
            h.update(repr(v).encode())
    add(value)
    return h.hexdigest()[:32]


class Runner:
    def __init__(self, out):
        self.out = out
        self.dev = torch.device("cuda", 0)
        self.cases = 0

    def engine(self, name, dtype, max_batch=250, chunk=None):
        return MCDEngine(model_of(name), self.dev, max_batch=max_batch, chunk_samples=chunk, dtype=dtype)

    def images(self, n=250):
        return synthetic_images(n, seed=1234).to(self.dev)

    def case(self, label, eng, call, note=None):
        eng.profile(True)
        r = call()
        torch.cuda.synchronize()
        eng.profile_read()
        rows = eng.profile_launches()
        eng.profile(False)
        table = hashlib.sha256(repr([(w["kind"], w["family"], w["out"], w["images"]) for w in rows]).encode()).hexdigest()[:32]
        self.out(f"{label:58s} launches={len(rows):4d} table={table} out={digest(r)}{note(r) if note else ''}")
        self.cases += 1

    def close(self, eng):
        eng.close()
        del eng
        torch.cuda.empty_cache()


def exit_threshold(eng, x, first_exit=1):
    """The (lower) median over the images of the T_EXIT-sample mean confidence at the first tested exit: the rule is strict (>), so about
    half of the images leave there and the others go on to the later exits."""
    mean = eng.predict(x, T_EXIT, seed=SEED)["mean"]
    return float(mean[first_exit].max(dim=1).values.median())


def sem_threshold(var, t):
    """The (lower) median over the images of the largest standard error max_c sqrt(var_c / t) of the last exit after the first step: about
    half of the images retire after the first step (whole-batch launches), the later steps run on the image list."""
    return float((var[-1] / t).sqrt().max(dim=1).values.median())


def dynamic_family(run, name, dtype):
    tag = f"{name}/{dtype}"
    eng, x = run.engine(name, dtype), run.images()
    E = eng.n_exits
    thr = exit_threshold(eng, x)
    sem = sem_threshold(eng.predict(x, T_STEP, seed=SEED)["var"], T_STEP)
    sem_ens = sem_threshold(eng.predict_ensemble(x, T_STEP, seed=SEED)["ens_var"], T_STEP)
    ex = lambda r: f" thr={thr!r} active_after={r['active_after']}"
    ad = lambda t: (lambda r: f" thr={t!r} active_after_step={r['active_after_step']}")

    def go(label, call, note):
        run.case(f"{label} {tag}", eng, call, note)

    go("predict_with_exit", lambda: eng.predict_with_exit(x, T_EXIT, thr, seed=SEED), ex)
    go("predict_early_exit readout=0", lambda: eng.predict_early_exit(x, T_EXIT, thr, seed=SEED), ex)
    go("predict_early_exit readout=1", lambda: eng.predict_early_exit(x, T_EXIT, thr, seed=SEED, ensemble_readout=True), ex)
    adaptive = lambda t, **kw: (lambda: eng.predict_adaptive(x, T_MAX, t, t_step=T_STEP, seed=SEED, **kw))
    go("predict_adaptive ensemble=0 stop_on=exit", adaptive(sem), ad(sem))
    go("predict_adaptive ensemble=1 stop_on=exit", adaptive(sem, ensemble=True), ad(sem))
    go("predict_adaptive ensemble=1 stop_on=ensemble", adaptive(sem_ens, ensemble=True, stop_on="ensemble"), ad(sem_ens))
    eng.set_ensemble_weights([float(i + 1) for i in range(E)])
    go("predict_early_exit weighted ensemble rule", lambda: eng.predict_early_exit(x, T_EXIT, thr, seed=SEED, ensemble=True, ensemble_readout=True), ex)
    go("predict_adaptive weighted stop_on=ensemble", adaptive(sem_ens, ensemble=True, stop_on="ensemble"), ad(sem_ens))
    run.close(eng)


def calibration_family(run, name="resnet18_me", dtype="f16", B=37, T=9):
    tag = f"{name}/{dtype} B={B} T={T}"
    eng, x = run.engine(name, dtype, max_batch=B, chunk=4), run.images(B)
    E, Cd = eng.n_exits, eng.out_dim
    rng = np.random.default_rng(7)
    tau = [1.5, 1.25, 0.8, 2.0, 0.6][:E]
    scale, vbias = np.linspace(0.5, 1.5, E * Cd).reshape(E, Cd), np.linspace(-0.25, 0.25, E * Cd).reshape(E, Cd)
    matrix = np.eye(Cd)[None] * scale[:, :, None] + rng.uniform(-0.1, 0.1, (E, Cd, Cd))
    weights = [float(i + 1) for i in range(E)]
    maps = (("temperature", eng.set_temperature, (tau,), dict(tau=tau)), ("vector", eng.set_vector_scaling, (scale, vbias), dict(scale=scale, bias=vbias)),
            ("matrix", eng.set_matrix_scaling, (matrix, vbias), dict(matrix=matrix, bias=vbias)))
    eng.set_matrix_scaling(matrix, vbias)
    run.case(f"predict_ensemble matrix {tag}", eng, lambda: eng.predict_ensemble(x, T, seed=SEED))
    eng.set_matrix_scaling(None)
    for kind, setter, args, _ in maps:
        setter(*args)
        for w in (None, weights):
            eng.set_ensemble_weights(w)
            run.case(f"predict_votes {kind} weights={int(w is not None)} {tag}", eng, lambda: eng.predict_votes(x, T, seed=SEED))
        setter(None)
    logits = eng.forward_samples(x, T, seed=SEED)
    labels = torch.from_numpy(rng.integers(0, Cd, B)).to(run.dev)
    for kind, _, _, kw in maps:
        for w in (None, weights):
            run.case(f"ensemble_moments {kind} weights={int(w is not None)} {tag}", eng, lambda: eng.ensemble_moments(logits, weights=w, **kw))
            run.case(f"vote_counts {kind} weights={int(w is not None)} {tag}", eng, lambda: eng.vote_counts(logits, weights=w, **kw))
    grid = np.exp(np.linspace(np.log(0.25), np.log(4.0), 7))[None].repeat(E, 0)
    run.case(f"nll_grid {tag}", eng, lambda: eng.nll_grid(logits, labels, grid))
    run.case(f"nll_vector_grad {tag}", eng, lambda: eng.nll_vector_grad(logits, labels, scale, vbias))
    run.case(f"nll_matrix_grad {tag}", eng, lambda: eng.nll_matrix_grad(logits, labels, matrix, vbias))
    run.case(f"ensemble_nll_grid {tag}", eng, lambda: eng.ensemble_nll_grid(logits, labels, tau, [0, E - 1], grid[0]))
    run.close(eng)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="", help="also write the lines to this file")
    ap.add_argument("--only", default="", choices=("", "calibration"), help="run this family of cases alone")
    a = ap.parse_args()
    f = open(a.out, "w") if a.out else None

    def out(line):
        print(line, flush=True)
        if f:
            f.write(line + "\n")
            f.flush()

    run = Runner(out)
    out(f"# {torch.cuda.get_device_name(0)}; ABI {_lib.lib().bmi_version()}")
    if a.only == "calibration":
        calibration_family(run)
        out(f"# done: {run.cases} cases")
        if f:
            f.close()
        return
    x = run.images()
    for name, dtype in PREDICT:
        eng = run.engine(name, dtype)
        run.case(f"predict {name}/{dtype} T={T_PREDICT} chunk={eng.chunk_samples}", eng, lambda: eng.predict(x, T_PREDICT, seed=SEED))
        run.close(eng)
    for name, opt, val, default in VARIANTS:
        _lib.set_option(opt, val)
        try:
            eng = run.engine(name, "f16")
            run.case(f"predict {name}/f16 {opt}={val} T={T_PREDICT}", eng, lambda: eng.predict(x, T_PREDICT, seed=SEED))
            run.close(eng)
        finally:
            _lib.set_option(opt, default)
    eng = run.engine("resnet18_masksembles", "f16")
    run.case("forward_samples mask_stride=3 resnet18_masksembles/f16", eng, lambda: eng.forward_samples(x, 8, seed=SEED, cnt0=1, mask_stride=3))
    run.close(eng)
    eng = run.engine("resnet18_me", "f16")
    E, Cd = eng.n_exits, eng.out_dim
    ens = lambda: eng.predict_ensemble(x, T_ENSEMBLE, seed=SEED)
    run.case(f"predict_ensemble plain resnet18_me/f16 T={T_ENSEMBLE}", eng, ens)
    eng.set_temperature([1.5, 1.25, 0.8, 2.0][:E])
    run.case(f"predict_ensemble temperature resnet18_me/f16 T={T_ENSEMBLE}", eng, ens)
    eng.set_temperature(None)
    eng.set_vector_scaling(np.linspace(0.5, 1.5, E * Cd).reshape(E, Cd), np.linspace(-0.25, 0.25, E * Cd).reshape(E, Cd))
    eng.set_ensemble_weights([float(i + 1) for i in range(E)])
    run.case(f"predict_ensemble vector+weights resnet18_me/f16 T={T_ENSEMBLE}", eng, ens)
    run.close(eng)
    for name, dtype in DYNAMIC:
        dynamic_family(run, name, dtype)
    xs = run.images(37)
    for name, dtype in SMALL:
        eng = run.engine(name, dtype, max_batch=37, chunk=4)
        run.case(f"predict {name}/{dtype} B=37 chunk=4 T=9", eng, lambda: eng.predict(xs, 9, seed=SEED))
        run.close(eng)
    for var, val in ENVS:
        os.environ[var] = val
        try:
            eng = run.engine("resnet18_me", "f16")
            run.case(f"predict resnet18_me/f16 {var}={val} T={T_PREDICT}", eng, lambda: eng.predict(x, T_PREDICT, seed=SEED))
            run.close(eng)
        finally:
            del os.environ[var]
    calibration_family(run)
    out(f"# done: {run.cases} cases")
    if f:
        f.close()


if __name__ == "__main__":
    main()
