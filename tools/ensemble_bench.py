#!/usr/bin/env python3
"""Same-process, interleaved A/B of ``predict_uncertainty`` (A) against ``predict_ensemble`` (B: the same heads, which also leave their
per-sample logits in the engine's scratch, plus one launch of csrc/ensemble.hip per chunk) on bench workloads: one engine, rounds of
``--steps`` timed steps of each, alternating, HIP events around each round.  A runs twice per round (A and A'): the spread between the
two is what a difference between A and B has to exceed to mean anything.

    python tools/ensemble_bench.py --workload resnet18_me resnet18_exit_only --rounds 15 --steps 20
    python tools/ensemble_bench.py --workload resnet18_exit_only --only B --rounds 3          (under rocprofv3 --kernel-trace --stats)
Prints per workload and variant the median / min / max ms per step over the rounds, and the per-kind launch times of one profiled
B step (bmi_profile_read: the batched head launch of the same step, to set the new kernel's time against).
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
    ap.add_argument("--rounds", type=int, default=15)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--dtype", default="f16")
    ap.add_argument("--only", choices=["A", "B"], default=None, help="run one variant alone (a profiler run)")
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
        run_a = lambda: eng.predict_uncertainty(x, T, seed=42)
        run_b = lambda: eng.predict_ensemble(x, T, seed=42)
        variants = {"A predict_uncertainty": run_a, "B predict_ensemble": run_b, "A' predict_uncertainty": run_a}
        if a.only:
            variants = {k: v for k, v in variants.items() if k.startswith(a.only + " ")}
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
        base = float(np.median(ms[next(iter(ms))]))
        for k, v in ms.items():
            med = float(np.median(v))
            print(f"{name:20s} {k:24s} median {med:8.4f} ms  min {min(v):8.4f}  max {max(v):8.4f}  ({100 * (med / base - 1):+.2f} % vs the first)  "
                  f"B={B} T={T} C={eng.out_dim} chunk={eng.chunk_samples} dtype={eng.dtype}")
        if a.only:
            continue
        # the new kernel against the heads of the same step: HIP events around the ensemble_moments launch alone, on the logits of this
        # engine, and the engine's own per-kind profile of one B step
        logits = eng.forward_samples(x, T, seed=42)
        for _ in range(3):
            eng.ensemble_moments(logits)
        lib, Q, QH = eng.lib, torch.zeros(2, *logits.shape[1:], dtype=torch.float64, device=dev), torch.zeros(*logits.shape[1:3], dtype=torch.float64, device=dev)
        st = eng._stream()
        t_k = []
        for _ in range(a.rounds):
            ev[0].record()
            for _ in range(a.steps):
                lib.bmi_ensemble_moments(logits.data_ptr(), T, logits.shape[1], B, logits.shape[3], None, Q[0].data_ptr(), Q[1].data_ptr(),
                                         QH.data_ptr(), st)
            ev[1].record()
            ev[1].synchronize()
            t_k.append(ev[0].elapsed_time(ev[1]) / a.steps)
        print(f"{name:20s} ensemble_moments_kernel alone (T={T} in one launch): median {np.median(t_k):8.4f} ms  min {min(t_k):8.4f}  max {max(t_k):8.4f}")
        eng.profile(True)
        run_b()
        prof = eng.profile_read()
        eng.profile(False)
        print(f"{name:20s} profile of one B step (bmi_profile_read, the ensemble launch is not a profiled op): {prof}")


if __name__ == "__main__":
    main()
