#!/usr/bin/env python3
"""Per-pass multi-exit accuracy on the device, measured.  One JSON line per measurement.

  (r) no GPU: the resource lines of pass_accuracy.hip's two kernels (tools/kernel_resources.py);
  (k) the device time of one MCDEngine.pass_accuracy call (its two launches, HIP events) against MultiExitAccuracy._metrics_passes (the torch
      route's dozen launches, which compute two of the 2 E rows) on the same logits;
  (w) the wall time of a whole evaluate() walk, device_metrics False against True, the two routes alternating in one process, a host clock
      around a call that ends in its own synchronisation; the returned vectors are compared (accuracy entries equal, avg_maxprob apart by
      the fp32 softmax's error).
  Both at the paper's size (resnet18 exit-only dropout, C = 100, T = 10, batch 250) and at the headline size (block + exit dropout, C = 10,
  T = 100, batch 250).  Medians over --rounds timings.

    python tools/pass_accuracy_bench.py [--rounds 9] [--launches 20] [--batches 8] [--parts k,w]
    python tools/pass_accuracy_bench.py --parts r
"""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from vector_scaling_bench import SIZES, event_ms, model_of, stats  # noqa: E402


def part_r(a):
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "kernel_resources.py"), "pass_accuracy.hip"], capture_output=True, text=True)
    if out.returncode:
        sys.exit(out.stderr[-2000:])
    cols = ("sgpr", "vgpr", "agpr", "scratch", "occ", "s_spill", "v_spill", "lds")
    for line in out.stdout.splitlines()[1:]:
        print(json.dumps(dict(part="r", kernel=line[:90].strip().split("(")[0], **{c: int(x) for c, x in zip(cols, line[90:].split())})), flush=True)


def part_k(a):
    from bayesnn_fpga_amd.synthetic import synthetic_images, synthetic_labels
    from bayesnn_fpga_amd.train.evaluate import MultiExitAccuracy
    dev = torch.device("cuda", 0)
    for tag, (kw, B, T) in SIZES.items():
        m = model_of(kw, dev)
        eng = m.engine(dev, max_batch=B, dtype="f16x2")
        E, C = eng.n_exits, eng.out_dim
        logits = eng.forward_samples(synthetic_images(B, seed=1234).to(dev), T, seed=1)
        y = synthetic_labels(B, C, seed=4).to(dev)
        y32 = y.to(torch.int32)
        loss = MultiExitAccuracy(E, acc_tops=(1, 5))
        out = eng.pass_accuracy(logits, y32)
        nf = torch.zeros(1, dtype=torch.int32, device=dev)
        fns = {"A torch _metrics_passes (2 rows)": lambda: loss._metrics_passes(logits, y),
               "B pass_accuracy (2 E rows)": lambda: eng.pass_accuracy(logits, y32, (1, 5), out=out, nonfinite=nf),
               "A' torch _metrics_passes (2 rows)": lambda: loss._metrics_passes(logits, y)}
        arms = list(fns)
        times = {k: [] for k in arms}
        for fn in fns.values():
            for _ in range(5):
                fn()
        torch.cuda.synchronize()
        for r in range(a.rounds):
            for k in (arms if r % 2 == 0 else arms[::-1]):
                times[k].append(event_ms(fns[k], a.launches))
        for k in arms:
            s = stats(times[k])
            print(json.dumps(dict(part="k", size=tag, what="read-out of one batch's logits, HIP events", arm=k, B=B, T=T, E=E, C=C,
                                  launches_per_timing=a.launches, timings=a.rounds, **s,
                                  ratio_to_A=round(s["median_ms"] / stats(times[arms[0]])["median_ms"], 4))), flush=True)


def part_w(a):
    from bayesnn_fpga_amd.synthetic import synthetic_images, synthetic_labels
    from bayesnn_fpga_amd.train.evaluate import MultiExitAccuracy, evaluate
    dev = torch.device("cuda", 0)
    for tag, (kw, B, T) in SIZES.items():
        m = model_of(kw, dev)
        m.engine_dtype = "f16x2"
        nb = a.batches
        x, y = synthetic_images(B * nb, seed=3), synthetic_labels(B * nb, kw["out_dim"], seed=4)
        loader = [(x[i * B:(i + 1) * B], y[i * B:(i + 1) * B]) for i in range(nb)]
        loss = MultiExitAccuracy(4, acc_tops=(1, 5))
        arms = ("A device_metrics=False", "B device_metrics=True", "A' device_metrics=False")
        times, vec = {k: [] for k in arms}, {}

        def walk(k):
            m.mc_pass = 0                                        # (the same draws for every walk)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            v = evaluate(loss, loader, m, 0, "bench", T, create_log=False, device_metrics=k.startswith("B"))
            torch.cuda.synchronize()
            return time.perf_counter() - t0, np.array(v)
        for k in arms[:2]:
            walk(k)                                              # warm-up: engines, buffers, code objects
        for r in range(a.rounds):
            for k in (arms if r % 2 == 0 else arms[::-1]):
                t, vec[k] = walk(k)
                times[k].append(t * 1e3)
        for k in arms:
            s = stats(times[k])
            print(json.dumps(dict(part="w", size=tag, what="evaluate() walk, host clock", arm=k, batches=nb, B=B, T=T, timings=a.rounds, **s,
                                  ms_per_batch=round(s["median_ms"] / nb, 4),
                                  ratio_to_A=round(s["median_ms"] / stats(times[arms[0]])["median_ms"], 4))), flush=True)
        print(json.dumps(dict(part="w", size=tag, what="the two routes' vectors", accuracy_entries_equal=bool(np.array_equal(vec[arms[0]][:-1], vec[arms[1]][:-1])),
                              avg_maxprob_difference=float(abs(vec[arms[0]][-1] - vec[arms[1]][-1])))), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--launches", type=int, default=20)
    ap.add_argument("--batches", type=int, default=8)
    ap.add_argument("--parts", default="k,w")
    a = ap.parse_args()
    parts = a.parts.split(",")
    if set(parts) - {"r"} and not torch.cuda.is_available():
        sys.exit("pass_accuracy_bench.py measures parts k and w on the GPU: none visible (--parts r needs none)")
    for p in parts:
        {"r": part_r, "k": part_k, "w": part_w}[p](a)


if __name__ == "__main__":
    main()
