#!/usr/bin/env python3
"""Conformal prediction sets on the device, measured.  One JSON line per measurement.

The classwise records of N images (E exits, C classes: R = 2 E rows, 4 R C bytes per image) sit on the device, as the walk leaves them.
  device  bmi_conformal_scores, bmi_conformal_quantile and bmi_conformal_sets (with and without the member words), each alone, device
          time by HIP events over --launches back-to-back calls, medians over --rounds; per method;
  host    what a caller does without them, under a host clock that starts behind a synchronisation: the records .cpu() (timed alone:
          the device-to-host copy), then train.conformal.conformal_numpy on the same arrays (timed alone).
The two routes' outputs are compared (equal bits).  Probabilities: a seeded softmax, right 60 % of the time.

    python tools/conformal_bench.py [--exits 4] [--classes 100] [--n 10000] [--rounds 9] [--launches 500]
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from vector_scaling_bench import event_ms, stats  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--exits", type=int, default=4)
    ap.add_argument("--classes", type=int, default=100)
    ap.add_argument("--n", type=int, default=10000)
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--launches", type=int, default=500)
    ap.add_argument("--host-rounds", type=int, default=2)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("conformal_bench.py measures on the GPU: none visible")
    from bayesnn_fpga_amd import _lib
    from bayesnn_fpga_amd.train.conformal import conformal_numpy
    lib, dev = _lib.lib(), torch.device("cuda", 0)
    E, Cd, N, coverage = a.exits, a.classes, a.n, (0.8, 0.9, 0.95)
    R, L, W = 2 * E, 3, (Cd + 31) // 32
    rng = np.random.default_rng(0)
    logits = rng.standard_normal((E, N, Cd)) * 2.0
    y = rng.integers(0, Cd, N)
    logits[:, np.arange(N), y] += (rng.random((E, N)) < 0.6) * 4.0
    p = np.exp(logits - logits.max(-1, keepdims=True))
    mean = torch.from_numpy(p / p.sum(-1, keepdims=True)).to(dev)
    labels = torch.from_numpy(y.astype(np.int32)).to(dev)
    pkeys = torch.full((R, Cd, N), -1, dtype=torch.int32, device=dev)
    rec = torch.full((N,), -1, dtype=torch.int32, device=dev)
    stream = lambda: C.c_void_p(torch.cuda.current_stream().cuda_stream)
    _lib.check(lib.bmi_classwise_record(mean.data_ptr(), E, N, Cd, labels.data_ptr(), 0, N, pkeys.data_ptr(), rec.data_ptr(), None, stream()),
               "bmi_classwise_record")
    scores = torch.empty(R, N, dtype=torch.int32, device=dev)
    qhat, n_valid = torch.empty(R, L, dtype=torch.int32, device=dev), torch.empty(R, dtype=torch.int64, device=dev)
    set_size = torch.empty(R, L, N, dtype=torch.uint8, device=dev)
    members = torch.empty(R, L, W, N, dtype=torch.int32, device=dev)
    shapes = dict(valid=(R,), covered=(R, L), size_sum=(R, L), size_hist=(R, L, Cd + 1), cov_hist=(R, L, Cd + 1), class_n=(R, Cd), class_cov=(R, L, Cd))
    t = {k: torch.empty(s, dtype=torch.int64, device=dev) for k, s in shapes.items()}
    levels = (C.c_double * L)(*coverage)
    host_in = None
    for name, k_reg, lam in (("lac", 0, 0.0), ("aps", 0, 0.0), ("raps", 5, 0.01)):
        code, lam_fix = _lib.CONFORMAL_METHODS[name], int(lam * 2 ** 30)

        def f_scores():
            _lib.check(lib.bmi_conformal_scores(pkeys.data_ptr(), rec.data_ptr(), R, Cd, N, N, code, k_reg, lam_fix, scores.data_ptr(), stream()), "scores")

        def f_quantile():
            _lib.check(lib.bmi_conformal_quantile(scores.data_ptr(), R, N, N, levels, L, qhat.data_ptr(), n_valid.data_ptr(), stream()), "quantile")

        def f_sets(words=True):
            _lib.check(lib.bmi_conformal_sets(pkeys.data_ptr(), rec.data_ptr(), R, Cd, N, N, code, k_reg, lam_fix, qhat.data_ptr(), L,
                                              set_size.data_ptr(), members.data_ptr() if words else None, *(v.data_ptr() for v in t.values()),
                                              stream()), "sets")

        arms = {"scores": f_scores, "quantile": f_quantile, "sets + members": f_sets, "sets": lambda: f_sets(False)}
        for fn in arms.values():
            fn()                                                                 # warm-up, and the later calls' inputs
        torch.cuda.synchronize()
        for arm, fn in arms.items():
            ts = [event_ms(fn, a.launches) for _ in range(a.rounds)]
            print(json.dumps(dict(what="device time, HIP events", method=name, call=arm, E=E, C=Cd, N=N, launches_per_timing=a.launches,
                                  timings=a.rounds, **stats(ts))), flush=True)
        f_sets()
        torch.cuda.synchronize()
        copies, hosts = [], []
        for _ in range(a.host_rounds):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            host_in = (pkeys.cpu().numpy(), rec.cpu().numpy())
            t1 = time.perf_counter()
            want = conformal_numpy(*host_in, name, k_reg, lam, coverage)
            copies.append((t1 - t0) * 1e3)
            hosts.append((time.perf_counter() - t1) * 1e3)
        got = dict(score_keys=scores, qhat=qhat, n_valid=n_valid, set_size=set_size, members=members, **t)
        same = all(np.array_equal(np.ascontiguousarray(v.cpu().numpy()).view(np.uint8), np.ascontiguousarray(want[k]).view(np.uint8))
                   for k, v in got.items())
        print(json.dumps(dict(what="host route, host clock", method=name, E=E, C=Cd, N=N, timings=a.host_rounds,
                              copy_bytes=int(pkeys.numel() * 4 + rec.numel() * 4), copy=stats(copies), conformal_numpy=stats(hosts),
                              outputs_equal=bool(same))), flush=True)


if __name__ == "__main__":
    main()
