#!/usr/bin/env python3
"""The exit-policy sweep on the device, measured against the host path for the same table.  One JSON line per measurement.

The T-mean probabilities [E, N, C] and the moment sums S1 of N images sit on the device (E = 4, C = 100, N = 10 000: the reference's test
sets).  Two routes to the threshold table alternate in one process under a host clock that starts behind a synchronisation and ends behind
the route's own last host read:
    A  the host path: the probabilities .cpu(), the exit ensembles on the host, then ``confidence_exiting.sweep`` — one numpy pass per
       threshold for accuracy, ECE, NLL and both FLOP counts, eleven thresholds;
    B  the device path: the records are on the device already (they are written per batch during the walk; their device time is
       reported separately), two ``exit_policy_sweep`` calls at G = 11 with the selected records (per exit and ensemble), two
       ``reliability_table`` calls on them, ``table_metrics`` and ``policy_metrics`` on the host (their reads: the synchronisation);
and, by HIP events, the device time of the record calls per batch, of one sweep at G = 11 with selected records and of one sweep at
G = 1024, counts only.  Medians over --rounds.

    python tools/exit_policy_bench.py [--rounds 9] [--launches 20] [--n 10000] [--batch 250] [--classes 100]
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from vector_scaling_bench import SIZES, event_ms, model_of, stats  # noqa: E402


def problem(E, N, Cd, T, seed=0):
    """Seeded softmax means of a network that grows more confident with depth, as sums of T samples: S1 float64 [E, N, C], labels [N]"""
    rng = np.random.default_rng(seed)
    y = rng.integers(0, Cd, N)
    logits = rng.standard_normal((E, N, Cd)) * 2.0
    logits[:, np.arange(N), y] += np.linspace(1.0, 4.0, E)[:, None] * (rng.random(N) < 0.7)
    p = np.exp(logits - logits.max(axis=2, keepdims=True))
    return p / p.sum(axis=2, keepdims=True) * T, y


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--launches", type=int, default=20)
    ap.add_argument("--n", type=int, default=10000)
    ap.add_argument("--batch", type=int, default=250)
    ap.add_argument("--classes", type=int, default=100)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("exit_policy_bench.py measures on the GPU: none visible")
    from bayesnn_fpga_amd.train import confidence_exiting as cex
    from bayesnn_fpga_amd.train.exit_policy import policy_metrics, reference_costs
    from bayesnn_fpga_amd.train.reliability import table_metrics
    from bayesnn_fpga_amd.train.results_analyzer import exit_ensembles
    dev = torch.device("cuda", 0)
    eng = model_of(SIZES["paper"][0], dev).engine(dev, max_batch=8, dtype="f16x2")      # (the read-out's methods live on an engine; no forward runs)
    E, N, Cd, B, T = eng.n_exits, a.n, a.classes, a.batch, 10
    S1, y = problem(E, N, Cd, T)
    Sd, yd = torch.from_numpy(S1).to(dev), torch.from_numpy(y)
    mean = (Sd * (1.0 / T)).contiguous()                     # finalize's mean
    onehot = np.eye(Cd)[y]
    cuts = [(o, min(B, N - o)) for o in range(0, N, B)]
    parts = [(Sd[:, o:o + b].contiguous(), mean[:, o:o + b].contiguous(), yd[o:o + b]) for o, b in cuts]
    rel, st = eng.new_reliability_records(N), eng.new_exit_stat_records(N)
    thr11 = torch.tensor(cex.CONFIDENCE_LIST, dtype=torch.float64, device=dev)
    thr1024 = torch.linspace(0.0, 1.0, 1024, dtype=torch.float64, device=dev)
    costs = [reference_costs("resnet18", True, T, ensembled=e) for e in (False, True)]

    def record():
        for (o, _), (s, m, lab) in zip(cuts, parts):
            eng.exit_stat_records(s, T, st, o)
            eng.reliability_records(m, lab, rel, o)

    def host():
        p = mean.cpu().numpy()
        rows = cex.sweep(p, exit_ensembles(p), onehot, "resnet18", True, T)
        return [(r["accuracy"], r["flops"], r["ens_accuracy"], r["ens_flops"]) for r in rows]

    def device():
        out = []
        for ens in (False, True):
            sw = eng.exit_policy_sweep(st, rel, N, thr11, ensemble=ens, select=True)
            m = table_metrics(eng.reliability_table(sw["selected"], N, 15, "mass", check=False), N)
            pm = policy_metrics(sw, costs[ens], N)
            out.append((pm["accuracy"], pm["cost"], m["ece"], m["nll"]))
        return [(float(out[0][0][g]), out[0][1][g], float(out[1][0][g]), out[1][1][g]) for g in range(len(thr11))]

    record()
    fns = {"A host: cpu() + confidence_exiting.sweep, 11 thresholds": host,
           "B device: 2 x (exit_policy_sweep G=11 with selected records + reliability_table) + host metrics": device,
           "A' host: cpu() + confidence_exiting.sweep, 11 thresholds": host}
    arms, vals = list(fns), {}
    times = {k: [] for k in arms}
    for k in arms[:2]:
        for _ in range(2):
            fns[k]()                                                             # warm-up: code objects, buffers, numpy's scratch
    for r in range(a.rounds):
        for k in (arms if r % 2 == 0 else arms[::-1]):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            vals[k] = fns[k]()
            times[k].append((time.perf_counter() - t0) * 1e3)
    for k in arms:
        s = stats(times[k])
        print(json.dumps(dict(what="threshold table from device-resident predictions, host clock", arm=k, N=N, E=E, C=Cd, timings=a.rounds, **s,
                              ratio_to_A=round(s["median_ms"] / stats(times[arms[0]])["median_ms"], 4))), flush=True)
    ha, da = vals[arms[0]], vals[arms[1]]
    print(json.dumps(dict(what="the two routes' numbers", N=N, rows_with_equal_accuracy_and_flops=sum(h == d for h, d in zip(ha, da)), rows=len(ha),
                          accuracy=[round(d[0], 4) for d in da], flops_rel=[round(d[1] / (cex.baseline_flops("resnet18") * N), 4) for d in da])),
          flush=True)
    torch.cuda.synchronize()
    for name, fn in ((f"records: {len(cuts)} x (exit_stat_records + reliability_records), one launch each", record),
                     ("sweep G=11 with selected records, two launches", lambda: eng.exit_policy_sweep(st, rel, N, thr11, select=True)),
                     ("sweep G=11 counts only", lambda: eng.exit_policy_sweep(st, rel, N, thr11)),
                     ("sweep G=1024 counts only, two launches", lambda: eng.exit_policy_sweep(st, rel, N, thr1024))):
        fn()
        ts = [event_ms(fn, a.launches) for _ in range(a.rounds)]
        print(json.dumps(dict(what="device time, HIP events (the outputs' allocation and zeroing included)", arm=name, N=N, E=E, batches=len(cuts),
                              launches_per_timing=a.launches, timings=a.rounds, **stats(ts))), flush=True)


if __name__ == "__main__":
    main()
