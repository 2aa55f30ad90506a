#!/usr/bin/env python3
"""Vote counts on the device, measured.  One JSON line per measurement.

  (r) no GPU: the resource lines of votes.hip's kernels (tools/kernel_resources.py);
  (k) the stand-alone launch (bmi_vote_counts, HIP events) on logits [100,4,250,10], [10,4,250,100] and [100,4,250,100] under every map,
      with the equal-weight and the weighted ensembles, against the yardstick: the ensemble_moments launch of csrc/ensemble.hip on the same
      logits under the same map (bmi_ensemble_moments*), the arms A / B / A' alternating in one process;
  (s) a whole step: MCDEngine.predict_ensemble against predict_votes, same process, at the headline size (block + exit dropout, C = 10,
      T = 100, batch 250) and at the paper's (exit-only dropout, C = 100, T = 10, batch 250): the added ms per step and its share.
  Medians over --rounds timings.

    python tools/votes_bench.py [--rounds 9] [--launches 20] [--parts k,s]
    python tools/votes_bench.py --parts r
"""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from vector_scaling_bench import SIZES, event_ms, model_of, stats  # noqa: E402

SHAPES = [(100, 4, 250, 10), (10, 4, 250, 100), (100, 4, 250, 100)]


def part_r(a):
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "kernel_resources.py"), "votes.hip"], capture_output=True, text=True)
    if out.returncode:
        sys.exit(out.stderr[-2000:])
    cols = ("sgpr", "vgpr", "agpr", "scratch", "occ", "s_spill", "v_spill", "lds")
    for line in out.stdout.splitlines()[1:]:
        print(json.dumps(dict(part="r", kernel=line[:90].strip().split("(")[0], **{c: int(x) for c, x in zip(cols, line[90:].split())})), flush=True)


def ab(fns, a):
    """Median / min / max ms per call of every arm, the arms alternating (the order reversed every other round)"""
    arms = list(fns)
    times = {k: [] for k in arms}
    for fn in fns.values():
        for _ in range(5):
            fn()
    torch.cuda.synchronize()
    for r in range(a.rounds):
        for k in (arms if r % 2 == 0 else arms[::-1]):
            times[k].append(event_ms(fns[k], a.launches))
    return {k: stats(times[k]) for k in arms}


def part_k(a):
    from bayesnn_fpga_amd import _lib
    lib = _lib.lib()
    dev = torch.device("cuda", 0)
    stream = lambda: C.c_void_p(torch.cuda.current_stream().cuda_stream)
    for T, E, B, Cd in SHAPES:
        rng = np.random.default_rng(T + Cd)
        logits = torch.from_numpy((3 * rng.standard_normal((T, E, B, Cd))).astype(np.float32)).to(dev)
        tau = (C.c_float * E)(*rng.uniform(0.5, 3.0, E).tolist())
        va = torch.from_numpy(rng.uniform(0.5, 2.0, (E, Cd)).astype(np.float32)).to(dev)
        vb = torch.from_numpy((0.5 * rng.standard_normal((E, Cd))).astype(np.float32)).to(dev)
        M = (0.05 * rng.standard_normal((E, Cd, Cd))).astype(np.float32)
        M[:, np.arange(Cd), np.arange(Cd)] = va.cpu().numpy()
        M = torch.from_numpy(M).to(dev)
        Wn = np.tril(rng.uniform(0.2, 1.0, (E, E)))
        W = torch.from_numpy(Wn / Wn.sum(1, keepdims=True)).to(dev)
        Q = torch.zeros(2, E, B, Cd, dtype=torch.float64, device=dev)
        QH = torch.zeros(E, B, dtype=torch.float64, device=dev)
        V = torch.zeros(2, E, B, Cd, dtype=torch.int32, device=dev)
        lp, q = logits.data_ptr(), (Q[0].data_ptr(), Q[1].data_ptr(), QH.data_ptr())
        for weighted in (False, True):
            w = W.data_ptr() if weighted else None
            ens = {"none": (lambda: lib.bmi_ensemble_moments_weighted(lp, T, E, B, Cd, None, w, *q, stream())) if weighted else
                           (lambda: lib.bmi_ensemble_moments(lp, T, E, B, Cd, None, *q, stream())),
                   "tau": (lambda: lib.bmi_ensemble_moments_weighted(lp, T, E, B, Cd, tau, w, *q, stream())) if weighted else
                          (lambda: lib.bmi_ensemble_moments(lp, T, E, B, Cd, tau, *q, stream())),
                   "vector": lambda: lib.bmi_ensemble_moments_vector(lp, T, E, B, Cd, va.data_ptr(), vb.data_ptr(), w, *q, stream()),
                   "matrix": lambda: lib.bmi_ensemble_moments_matrix(lp, T, E, B, Cd, M.data_ptr(), vb.data_ptr(), w, *q, stream())}
            maps = {"none": (None, None, None, None), "tau": (tau, None, None, None), "vector": (None, va.data_ptr(), vb.data_ptr(), None),
                    "matrix": (None, None, vb.data_ptr(), M.data_ptr())}
            for kind in ("none", "tau", "vector", "matrix"):
                vote = lambda m=maps[kind]: lib.bmi_vote_counts(lp, T, E, B, Cd, *m, w, V.data_ptr(), None, stream())
                assert ens[kind]() == 0 and vote() == 0
                res = ab({"A ensemble_moments": ens[kind], "B vote_counts": vote, "A' ensemble_moments": ens[kind]}, a)
                base = res["A ensemble_moments"]["median_ms"]
                for k, s in res.items():
                    print(json.dumps(dict(part="k", shape=[T, E, B, Cd], map=kind, weighted=weighted, arm=k, launches_per_timing=a.launches,
                                          timings=a.rounds, **s, ratio_to_A=round(s["median_ms"] / base, 4))), flush=True)


def part_s(a):
    from bayesnn_fpga_amd.synthetic import synthetic_images
    dev = torch.device("cuda", 0)
    for tag, (kw, B, T) in SIZES.items():
        m = model_of(kw, dev)
        eng = m.engine(dev, max_batch=B, dtype="f16")
        x = synthetic_images(B, seed=1234).to(dev)
        S, H, Q, QH = eng.new_ensemble_sums(B)
        V = eng.new_vote_counts(B)
        fns = {"A accumulate_ensemble": lambda: eng.accumulate_ensemble(x, S, H, Q, QH, 0, T, 1),
               "B accumulate_votes": lambda: eng.accumulate_votes(x, S, H, Q, QH, V, 0, T, 1),
               "A' accumulate_ensemble": lambda: eng.accumulate_ensemble(x, S, H, Q, QH, 0, T, 1)}
        saved, a.launches = a.launches, max(1, a.launches // 4)
        res = ab(fns, a)
        a.launches = saved
        base = res["A accumulate_ensemble"]["median_ms"]
        for k, s in res.items():
            print(json.dumps(dict(part="s", size=tag, what="one step of T passes over the batch, HIP events", arm=k, B=B, T=T, E=eng.n_exits,
                                  C=eng.out_dim, chunk=eng.chunk_samples, timings=a.rounds, **s, added_ms=round(s["median_ms"] - base, 4),
                                  ratio_to_A=round(s["median_ms"] / base, 4))), flush=True)
        fin = ab({"finalize_votes": lambda: eng.finalize_votes(V)}, a)["finalize_votes"]
        print(json.dumps(dict(part="s", size=tag, what="the read-out of V (bmi_finalize_votes + its output allocations)", **fin)), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--launches", type=int, default=20)
    ap.add_argument("--parts", default="k,s")
    a = ap.parse_args()
    parts = a.parts.split(",")
    if set(parts) - {"r"} and not torch.cuda.is_available():
        sys.exit("votes_bench.py measures parts k and s on the GPU: none visible (--parts r needs none)")
    for p in parts:
        {"r": part_r, "k": part_k, "s": part_s}[p](a)


if __name__ == "__main__":
    main()
