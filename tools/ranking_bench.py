#!/usr/bin/env python3
"""Rank quality on the device, measured.  One JSON line per measurement.

  (r) no GPU: the resource lines of ranking.hip's kernels (tools/kernel_resources.py);
  (t) the AUROC and the risk-coverage curve of R = 2 E rows of N per-image scores that sit on the device, float64 [R, N], with the hit bits
      beside them, two routes alternating in one process under a host clock that starts behind a synchronisation and ends behind the
      route's own last host read:
        A  what a caller of the engine does without this read-out: the scores and the bits .cpu(), then per row
           np.argsort(kind="stable"), cumsum for the curve, the tie groups by searchsorted on the sorted scores for the Mann-Whitney
           count, the AURC sum vectorised;
        B  MCDEngine.score_records per batch of --batch images, ONE rank_quality, rank_metrics on the host (its reads of counts and
           aurc_sum: the synchronisation);
      and the device time of B's two halves, and of the rank call alone, by HIP events.  The two routes' numbers are compared.
  Sizes: --n 10000 (the reference's test sets; E = 4, R = 8) and --n 131072 (the largest row the rank call takes).  Medians over --rounds.

    python tools/ranking_bench.py [--rounds 9] [--launches 20] [--n 10000] [--batch 250] [--parts t]
    python tools/ranking_bench.py --parts r
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
    cols = ("sgpr", "vgpr", "agpr", "scratch", "occ", "s_spill", "v_spill", "lds")
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "kernel_resources.py"), "ranking.hip"], capture_output=True, text=True)
    if out.returncode:
        sys.exit(out.stderr[-2000:])
    for line in out.stdout.splitlines()[1:]:
        print(json.dumps(dict(part="r", kernel=line[:90].strip().split("(")[0], **{c: int(x) for c, x in zip(cols, line[90:].split())})),
              flush=True)


def problem(R, N, seed=0):
    """Seeded entropies of a network that is right 60 % of the time and more certain when right: float64 [R, N], hit uint8 [R, N]"""
    rng = np.random.default_rng(seed)
    hit = (rng.random((R, N)) < 0.6).astype(np.uint8)
    score = np.abs(rng.standard_normal((R, N)) * 0.5 + np.where(hit, 0.6, 1.3))
    return score, hit


def host_route(score, hit):
    """-> (auroc [R], aurc [R]) with numpy on the host: the stable order, the curve, ties counted half"""
    s32 = score.astype(np.float32)
    auroc, aurc = [], []
    for r in range(s32.shape[0]):
        order = np.argsort(s32[r], kind="stable")
        pos = 1 - hit[r][order].astype(np.int64)
        cum = np.cumsum(pos)
        su = s32[r][order]
        neg_cum = np.cumsum(1 - pos)
        first, last = np.searchsorted(su, su, side="left"), np.searchsorted(su, su, side="right")
        before = np.where(first > 0, neg_cum[np.maximum(first - 1, 0)], 0)
        u2 = int((pos * (before + neg_cum[last - 1])).sum())
        n_pos = int(cum[-1])
        auroc.append(u2 / (2.0 * n_pos * (len(pos) - n_pos)))
        aurc.append(float((cum / np.arange(1, len(cum) + 1)).sum()) / len(cum))
    return np.array(auroc), np.array(aurc)


def part_t(a):
    from bayesnn_fpga_amd.train.ranking import rank_metrics
    dev = torch.device("cuda", 0)
    eng = model_of(SIZES["paper"][0], dev).engine(dev, max_batch=8, dtype="f16x2")      # (the read-out's methods live on an engine; no forward runs)
    R, N, B = 2 * eng.n_exits, a.n, a.batch
    score, hit = problem(R, N)
    sd, hd = torch.from_numpy(score).to(dev), torch.from_numpy(hit).to(dev)
    positive = (1 - hd).contiguous()
    cuts = [(o, min(B, N - o)) for o in range(0, N, B)]
    parts = [sd[:, o:o + b].contiguous() for o, b in cuts]                       # what predict_votes hands over, batch by batch
    rec = eng.new_score_records(N, R)

    def host():
        return host_route(sd.cpu().numpy(), hd.cpu().numpy())

    def record():
        for (o, _), p in zip(cuts, parts):
            eng.score_records(p, rec, o, 1)

    def device():
        record()
        m = rank_metrics(eng.rank_quality(rec["ukeys"], positive, N))
        return m["auroc"], m["aurc"]

    fns = {"A host: cpu() + R x (stable argsort + cumsum + tie groups)": host, "B device: score_records per batch + one rank_quality": device,
           "A' host: cpu() + R x (stable argsort + cumsum + tie groups)": host}
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
        print(json.dumps(dict(part="t", what="AUROC and AURC rows from device-resident scores, host clock", arm=k, N=N, R=R, batch=B,
                              timings=a.rounds, **s, ratio_to_A=round(s["median_ms"] / stats(times[arms[0]])["median_ms"], 4))), flush=True)
    (a_roc, a_rc), (b_roc, b_rc) = vals[arms[0]], vals[arms[1]]
    print(json.dumps(dict(part="t", what="the two routes' numbers", N=N, max_auroc_difference=float(np.abs(a_roc - b_roc).max()),
                          max_rel_aurc_difference=float((np.abs(a_rc - b_rc) / a_rc).max()), auroc=[round(float(v), 6) for v in b_roc])),
          flush=True)
    torch.cuda.synchronize()
    for name, fn in ((f"records: {len(cuts)} score_records calls, one launch each", record),
                     ("rank: one rank_quality, two launches", lambda: eng.rank_quality(rec["ukeys"], positive, N))):
        ts = [event_ms(fn, a.launches) for _ in range(a.rounds)]
        print(json.dumps(dict(part="t", what="device time, HIP events", arm=name, N=N, R=R, batches=len(cuts), launches_per_timing=a.launches,
                              timings=a.rounds, **stats(ts), pair_steps_per_ns=round(R * N * N / (stats(ts)["median_ms"] * 1e6), 2)
                              if name.startswith("rank") else None)), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--launches", type=int, default=20)
    ap.add_argument("--n", type=int, default=10000)
    ap.add_argument("--batch", type=int, default=250)
    ap.add_argument("--parts", default="t")
    a = ap.parse_args()
    parts = a.parts.split(",")
    if set(parts) - {"r"} and not torch.cuda.is_available():
        sys.exit("ranking_bench.py measures part t on the GPU: none visible (--parts r needs none)")
    for p in parts:
        {"r": part_r, "t": part_t}[p](a)


if __name__ == "__main__":
    main()
