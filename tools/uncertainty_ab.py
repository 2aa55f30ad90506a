#!/usr/bin/env python3
"""Same-process, interleaved A/B of ``predict`` against ``predict_uncertainty`` (the fused heads' entropy path) on bench workloads:
one engine, rounds of ``--steps`` timed steps of each, alternating, HIP events around each round.

    python tools/uncertainty_ab.py --workload resnet18_me resnet18_exit_only --rounds 9 --steps 5
Prints per workload and variant the median / min / max ms per step over the rounds and the median overhead.
"""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402
from bayesnn_fpga_amd.synthetic import synthetic_images, synthetic_weights_  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", nargs="+", default=["resnet18_me", "resnet18_exit_only"], choices=sorted(bench.WORKLOADS))
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--dtype", default="f16")
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    for name in a.workload:
        wl = bench.WORKLOADS[name]
        torch.manual_seed(0)
        np.random.seed(0)
        model = synthetic_weights_(bench._load(wl[0])(**wl[2]), 0).to(dev).eval()
        B, T = wl[3], wl[4]
        x = synthetic_images(B, seed=1234).to(dev)
        eng = model.engine(dev, max_batch=B, dtype=a.dtype)
        variants = {"predict": lambda: eng.predict(x, T, seed=42), "predict_uncertainty": lambda: eng.predict_uncertainty(x, T, seed=42)}
        for fn in variants.values():
            for _ in range(3):
                fn()
        torch.cuda.synchronize()
        ms = {k: [] for k in variants}
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
        for r in range(a.rounds):
            order = list(variants) if r % 2 == 0 else list(variants)[::-1]
            for k in order:
                ev[0].record()
                for _ in range(a.steps):
                    variants[k]()
                ev[1].record()
                ev[1].synchronize()
                ms[k].append(ev[0].elapsed_time(ev[1]) / a.steps)
        eng.check_finite()
        base = float(np.median(ms["predict"]))
        for k, v in ms.items():
            med = float(np.median(v))
            print(f"{name:20s} {k:20s} median {med:8.3f} ms  min {min(v):8.3f}  max {max(v):8.3f}  "
                  f"({100 * (med / base - 1):+.1f} % vs predict)  B={B} T={T} dtype={eng.dtype}")


if __name__ == "__main__":
    main()
