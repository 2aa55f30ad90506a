#!/usr/bin/env python3
"""Weighted exit ensembles, measured.  One JSON line per measurement.

  (r) no GPU: the resource lines of the four instantiations of ensemble_moments_kernel (tools/kernel_resources.py ensemble.hip);
  (a) the weighted launch against the unweighted launch ON THE SAME LOGITS, straight through the C ABI on buffers made once, at the
      headline size (ResNet-18 multi-exit, B = 250, T = 100, C = 10) and at the paper's size (exit-only dropout, B = 250, T = 10,
      C = 100): HIP-event medians over alternating runs, each timing a run of launches between two events; the unweighted arm runs twice
      per round (A and A'), their spread is what a difference has to exceed; and predict_ensemble end to end with and without weights;
  (b) what the fit changes: on the trained-like twin (classifiers x 24; teacher labels drawn at tau* = 3 from the final exit, as
      tests/test_temperature.py draws them) the validation NLL of every ensemble row at equal weights and at the fitted weights, every exit
      alone, the fitted matrix and the EM iterations — at tau = 1 and, in the documented order, at the per-exit fitted temperatures.

    python tools/weighted_ensemble_bench.py [--rounds 9] [--launches 20] [--parts a,b]
    python tools/weighted_ensemble_bench.py --parts r
"""
import argparse
import json
import os
import subprocess
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HEADS = ("ex1linear", "ex2linear", "ex3linear", "linear")
SIZES = {"headline": (dict(dropout_exit=True, dropout="block", dropout_p=0.25, out_dim=10), 250, 100),
         "paper": (dict(dropout_exit=True, dropout=None, dropout_p=0.25, out_dim=100), 250, 10)}


def model_of(kw, dev, gain=None):
    from bayesnn_fpga_amd.models.resnet18.resnet18 import ResNet18MCEarlyExit
    from bayesnn_fpga_amd.synthetic import synthetic_weights_
    torch.manual_seed(0)
    np.random.seed(0)
    m = synthetic_weights_(ResNet18MCEarlyExit(**kw), 0)
    if gain:
        with torch.no_grad():
            for n in HEADS:
                getattr(m, n).weight.mul_(gain)
    return m.to(dev).eval()


def event_ms(fn, launches):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(launches):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / launches


def stats(ts):
    ts = sorted(ts)
    return dict(median_ms=round(ts[len(ts) // 2], 4), min_ms=round(ts[0], 4), max_ms=round(ts[-1], 4))


def part_r(a):
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "kernel_resources.py"), "ensemble.hip"], capture_output=True, text=True)
    if out.returncode:
        sys.exit(out.stderr[-2000:])
    for line in out.stdout.splitlines():
        if "ensemble_moments_kernel" in line or line.startswith("kernel"):
            print(json.dumps(dict(part="r", line=" ".join(line.split()))), flush=True)


def part_a(a):
    from bayesnn_fpga_amd.synthetic import synthetic_images
    dev = torch.device("cuda", 0)
    for tag, (kw, B, T) in SIZES.items():
        m = model_of(kw, dev)
        eng = m.engine(dev, max_batch=B, dtype="f16")
        x = synthetic_images(B, seed=1234).to(dev)
        logits = eng.forward_samples(x, T, seed=1)
        E, C = eng.n_exits, eng.out_dim
        W = torch.from_numpy(np.tril(np.random.default_rng(0).random((E, E)) + 0.1)).to(dev)
        W = (W / W.sum(1, keepdim=True)).contiguous()
        Q = torch.zeros(2, E, B, C, dtype=torch.float64, device=dev)
        QH = torch.zeros(E, B, dtype=torch.float64, device=dev)
        lib, st = eng.lib, eng._stream()

        def plain():
            return lib.bmi_ensemble_moments(logits.data_ptr(), T, E, B, C, None, Q[0].data_ptr(), Q[1].data_ptr(), QH.data_ptr(), st)

        def weighted():
            return lib.bmi_ensemble_moments_weighted(logits.data_ptr(), T, E, B, C, None, W.data_ptr(), Q[0].data_ptr(), Q[1].data_ptr(),
                                                     QH.data_ptr(), st)
        assert plain() == 0 and weighted() == 0
        arms = {"A unweighted launch": plain, "B weighted launch": weighted, "A' unweighted launch": plain}
        times = {k: [] for k in arms}
        for fn in arms.values():
            for _ in range(5):
                fn()
        torch.cuda.synchronize()
        for r in range(a.rounds):
            for k in (list(arms) if r % 2 == 0 else list(arms)[::-1]):
                times[k].append(event_ms(arms[k], a.launches))
        base = stats(times["A unweighted launch"])["median_ms"]
        for k in arms:
            s = stats(times[k])
            print(json.dumps(dict(part="a", size=tag, what=k, B=B, T=T, E=E, C=C, launches_per_timing=a.launches, timings=a.rounds, **s,
                                  ratio_to_A=round(s["median_ms"] / base, 4))), flush=True)
        # end to end: the same engine with and without weights, alternating
        e2e = {"predict_ensemble": [], "predict_ensemble, weighted": []}
        for r in range(max(3, a.rounds // 3)):
            for k in e2e:
                eng.set_ensemble_weights(W if "weighted" in k else None)
                eng.predict_ensemble(x, T, seed=42)
                e2e[k].append(event_ms(lambda: eng.predict_ensemble(x, T, seed=42), 3))
        eng.set_ensemble_weights(None)
        eng.check_finite()
        for k, v in e2e.items():
            print(json.dumps(dict(part="a", size=tag, what=k, B=B, T=T, E=E, C=C, chunk=eng.chunk_samples, **stats(v))), flush=True)


def part_b(a):
    from bayesnn_fpga_amd.synthetic import synthetic_images
    from bayesnn_fpga_amd.train.calibration import EnsembleWeights, TemperatureScaling, temper_logits
    dev = torch.device("cuda", 0)
    sizes, T, seed = [250, 250, 250, 250], 10, 5
    x = synthetic_images(sum(sizes), seed=31)
    offs = np.concatenate([[0], np.cumsum(sizes)])
    for dropout, C in (("block", 10), (None, 100)):
        kw = dict(dropout_exit=True, dropout=dropout, dropout_p=0.25, out_dim=C)
        m = model_of(kw, dev, gain=24.0)
        m.engine_dtype = "f16x2"
        eng = m.engine(dev, max_batch=max(sizes))
        raw = np.concatenate([eng.forward_samples(x[offs[k]:offs[k + 1]].to(dev), T, seed=seed + k).cpu().numpy() for k in range(len(sizes))],
                             axis=2)
        rng = np.random.default_rng(7)
        labels = np.array([rng.choice(C, p=q / q.sum()) for q in temper_logits(raw, 3.0)[0][-1]])
        y = torch.from_numpy(labels)
        loader = [(x[offs[k]:offs[k + 1]], y[offs[k]:offs[k + 1]]) for k in range(len(sizes))]
        rd = lambda v: [round(float(t), 4) for t in np.asarray(v).reshape(-1)]       # noqa: E731
        for when in ("tau = 1", "per-exit fitted temperatures"):
            if when != "tau = 1":
                ts = TemperatureScaling(m, loader, gpu=0, mc_passes=T, seed=seed)
                ts.fit()
                ts.apply()
            r = EnsembleWeights(m, loader, gpu=0, mc_passes=T, seed=seed).fit()
            print(json.dumps(dict(part="b", model="x24 twin", dropout="block + exit" if dropout else "exit-only", C=C, n=r["n"], members=when,
                                  tau=rd(m.exit_temperature or [1.0] * 4), nll_per_exit=rd(r["nll_per_exit"]), nll_equal_weights=rd(r["nll_uniform"]),
                                  nll_fitted_weights=rd(r["nll_after"]), weights=[rd(row) for row in r["weights"]],
                                  em_iterations=[int(i) for i in r["iterations"]], converged=[bool(c) for c in r["converged"]])), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--launches", type=int, default=20)
    ap.add_argument("--parts", default="a,b")
    a = ap.parse_args()
    parts = a.parts.split(",")
    if set(parts) - {"r"} and not torch.cuda.is_available():
        sys.exit("weighted_ensemble_bench.py measures parts a and b on the GPU: none visible (--parts r needs none)")
    for p in parts:
        {"r": part_r, "a": part_a, "b": part_b}[p](a)


if __name__ == "__main__":
    main()
