#!/usr/bin/env python3
"""Reliability tables on the device, measured.  One JSON line per measurement.

  (r) no GPU: the resource lines of reliability.hip's kernels (tools/kernel_resources.py);
  (t) the calibration rows of N images from T-mean probabilities that sit on the device, float64 [E, N, C], two routes alternating in one
      process under a host clock that starts behind a synchronisation and ends behind the route's own last host read:
        A  the host route of FullAnalysis.all_experiments(ece="hist"): preds.cpu(), exit_ensembles, then ece_hist_binary + nll_mse_acc
           once per row, 2 E times;
        B  the device route of ReliabilityAnalysis: MCDEngine.reliability_records per batch of --batch images, ONE reliability_table
           (which reads the counters: the synchronisation), table_metrics on the host;
      and the device time of B's two halves by HIP events.  The two routes' rows are compared.
  (k) the KDE-ECE of the R = 2 E rows on --grid grid points (default 2^14), from records that sit on the device: ONE
      MCDEngine.reliability_kde call (three launches) by HIP events and under the host clock (with its host read of the degenerate flags),
      next to the host route of FullAnalysis.all_experiments(ece="kde"): preds.cpu(), exit_ensembles, then ece_kde_binary(method="fft") once
      per row, 2 E times.  The two routes' values are compared.
  (c) the classwise tables (bmi_classwise_record / bmi_classwise_table) by HIP events: classwise_records per batch next to
      reliability_records on the same means, ONE classwise_table by width and by mass; and under the host clock the host route it
      replaces — the float64 means copied to the host (timed alone), then a vectorised numpy classwise histogram (timed alone).  The two
      routes' classwise ECE are compared.
  (w) the ReliabilityAnalysis walk per batch on the seeded ResNet-18, --batch images per batch, T = 10, four batches: classwise=False
      against classwise=True, alternating, host clock around the whole walk divided by the batches.
  Default size: N = 10000, E = 4, C = 100 (CIFAR-100's test set through resnet18's four exits).  Medians over --rounds timings.

    python tools/reliability_bench.py [--rounds 9] [--launches 20] [--n 10000] [--classes 100] [--batch 250] [--grid 16384] [--parts t,k]
    python tools/reliability_bench.py --parts r
    python tools/reliability_bench.py --parts c,w --rounds 21
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
    for src in ("reliability.hip", "reliability_kde.hip", "reliability_classwise.hip"):
        out = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "kernel_resources.py"), src], capture_output=True, text=True)
        if out.returncode:
            sys.exit(out.stderr[-2000:])
        for line in out.stdout.splitlines()[1:]:
            print(json.dumps(dict(part="r", kernel=line[:90].strip().split("(")[0], **{c: int(x) for c, x in zip(cols, line[90:].split())})),
                  flush=True)


def problem(E, N, C, seed=0):
    """Seeded probabilities of a network that is right 60 % of the time: float64 [E, N, C] and labels [N]"""
    rng = np.random.default_rng(seed)
    l = rng.standard_normal((E, N, C)) * 3.0
    y = rng.integers(0, C, N)
    l[:, np.arange(N), y] += (rng.random((E, N)) < 0.6) * 6.0
    ex = np.exp(l - l.max(-1, keepdims=True))
    return ex / ex.sum(-1, keepdims=True), y


def part_t(a):
    from bayesnn_fpga_amd.train.metrics import ece_hist_binary, nll_mse_acc
    from bayesnn_fpga_amd.train.reliability import table_metrics
    from bayesnn_fpga_amd.train.results_analyzer import exit_ensembles
    dev = torch.device("cuda", 0)
    eng = model_of(SIZES["paper"][0], dev).engine(dev, max_batch=8, dtype="f16x2")      # (the read-out's methods live on an engine; no forward runs)
    E, N, C, B = eng.n_exits, a.n, a.classes, a.batch
    p, y = problem(E, N, C)
    preds, labels = torch.from_numpy(p).to(dev), torch.from_numpy(y).to(dev)
    onehot = np.zeros((N, C))
    onehot[np.arange(N), y] = 1
    cuts = [(o, min(B, N - o)) for o in range(0, N, B)]
    means = [preds[:, o:o + b].contiguous() for o, b in cuts]                    # what finalize() hands over, batch by batch
    ys = [labels[o:o + b].to(torch.int32) for o, b in cuts]
    rec = eng.new_reliability_records(N, n_exits=E)

    def host():
        pr = preds.cpu().numpy()
        rows = []
        for v in list(pr) + list(exit_ensembles(pr)):
            nll, mse, acc = nll_mse_acc(v, onehot)
            rows.append((acc, ece_hist_binary(v, onehot), nll, mse))
        return np.array(rows)

    def record():
        for (o, _), m, yy in zip(cuts, means, ys):
            eng.reliability_records(m, yy, rec, o)

    def device():
        record()
        m = table_metrics(eng.reliability_table(rec, N), N)
        return np.stack([m["acc"], m["ece"], m["nll"], m["brier"]], axis=1)

    fns = {"A host: cpu() + 2E x (ece_hist_binary + nll_mse_acc)": host, "B device: records per batch + one table": device,
           "A' host: cpu() + 2E x (ece_hist_binary + nll_mse_acc)": host}
    arms, rows = list(fns), {}
    times = {k: [] for k in arms}
    for k in arms[:2]:
        for _ in range(2):
            fns[k]()                                                             # warm-up: code objects, buffers, numpy's scratch
    for r in range(a.rounds):
        for k in (arms if r % 2 == 0 else arms[::-1]):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            rows[k] = fns[k]()
            times[k].append((time.perf_counter() - t0) * 1e3)
    for k in arms:
        s = stats(times[k])
        print(json.dumps(dict(part="t", what="calibration rows from device-resident preds, host clock", arm=k, N=N, E=E, C=C, batch=B,
                              timings=a.rounds, **s, ratio_to_A=round(s["median_ms"] / stats(times[arms[0]])["median_ms"], 4))), flush=True)
    d = np.abs(rows[arms[0]] - rows[arms[1]])
    print(json.dumps(dict(part="t", what="the two routes' rows", acc_equal=bool((d[:, 0] == 0).all()), max_ece_difference=float(d[:, 1].max()),
                          max_rel_nll_difference=float((d[:, 2] / rows[arms[0]][:, 2]).max()),
                          max_rel_brier_difference=float((d[:, 3] / rows[arms[0]][:, 3]).max()))), flush=True)
    torch.cuda.synchronize()
    for name, fn in (("records: one launch per batch", record), ("table: four launches", lambda: eng.reliability_table(rec, N, check=False))):
        ts = [event_ms(fn, a.launches) for _ in range(a.rounds)]
        print(json.dumps(dict(part="t", what="device time, HIP events", arm=name, N=N, E=E, C=C, batches=len(cuts),
                              launches_per_timing=a.launches, timings=a.rounds, **stats(ts))), flush=True)


def part_k(a):
    from bayesnn_fpga_amd.train.metrics import ece_kde_binary
    from bayesnn_fpga_amd.train.results_analyzer import exit_ensembles
    dev = torch.device("cuda", 0)
    eng = model_of(SIZES["paper"][0], dev).engine(dev, max_batch=8, dtype="f16x2")      # (no forward runs)
    E, N, C, B, G = eng.n_exits, a.n, a.classes, a.batch, a.grid
    p, y = problem(E, N, C)
    preds, labels = torch.from_numpy(p).to(dev), torch.from_numpy(y).to(dev)
    onehot = np.zeros((N, C))
    onehot[np.arange(N), y] = 1
    rec = eng.new_reliability_records(N, n_exits=E)
    for o in range(0, N, B):
        eng.reliability_records(preds[:, o:o + B].contiguous(), labels[o:o + B].to(torch.int32), rec, o)

    def host():
        pr = preds.cpu().numpy()
        return np.array([ece_kde_binary(v, onehot, grid_points=G, method="fft") for v in list(pr) + list(exit_ensembles(pr))])

    def device():
        return eng.reliability_kde(rec, N, G)["ece_kde"].cpu().numpy()

    fns = {"A host: cpu() + 2E x ece_kde_binary(method='fft')": host, "B device: one reliability_kde on the records": device}
    times, vals = {k: [] for k in fns}, {}
    device()
    for r in range(a.rounds):
        for k in (list(fns) if r % 2 == 0 else list(fns)[::-1]):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            vals[k] = fns[k]()
            times[k].append((time.perf_counter() - t0) * 1e3)
    for k in fns:
        print(json.dumps(dict(part="k", what="KDE-ECE rows, host clock", arm=k, N=N, R=2 * E, C=C, G=G, timings=a.rounds, **stats(times[k]))),
              flush=True)
    a_, b_ = (vals[k] for k in fns)
    print(json.dumps(dict(part="k", what="the two routes' values", max_difference=float(np.abs(a_ - b_).max()), device=[float(v) for v in b_])),
          flush=True)
    ts = [event_ms(lambda: eng.reliability_kde(rec, N, G, check=False), a.launches) for _ in range(a.rounds)]
    print(json.dumps(dict(part="k", what="device time, HIP events", arm="reliability_kde(check=False): three launches", N=N, R=2 * E, G=G,
                          launches_per_timing=a.launches, timings=a.rounds, **stats(ts))), flush=True)


def part_c(a):
    from bayesnn_fpga_amd.train.reliability import classwise_metrics, width_edges
    dev = torch.device("cuda", 0)
    eng = model_of(SIZES["paper"][0], dev).engine(dev, max_batch=8, dtype="f16x2")      # (no forward runs)
    E, N, C, B, nb = eng.n_exits, a.n, a.classes, a.batch, 15
    p, y = problem(E, N, C)
    preds, labels = torch.from_numpy(p).to(dev), torch.from_numpy(y).to(dev)
    cuts = [(o, min(B, N - o)) for o in range(0, N, B)]
    means = [preds[:, o:o + b].contiguous() for o, b in cuts]
    ys = [labels[o:o + b].to(torch.int32) for o, b in cuts]
    rec, cw = eng.new_reliability_records(N, n_exits=E), eng.new_classwise_records(N, n_exits=E, out_dim=C)
    print(json.dumps(dict(part="c", what="record bytes", pkeys_bytes=cw["pkeys"].numel() * 4, per_image=8 * E * C, top_label_per_image=21 * 2 * E)),
          flush=True)

    def one_top():
        eng.reliability_records(means[0], ys[0], rec, 0)

    def one_cw():
        eng.classwise_records(means[0], ys[0], cw, 0)

    for (o, _), m, yy in zip(cuts, means, ys):
        eng.classwise_records(m, yy, cw, o)
    arms = (("reliability_records, one batch", one_top), ("classwise_records, one batch", one_cw),
            ("classwise_table width", lambda: eng.classwise_table(cw, N, nb, "width", check=False)),
            ("classwise_table mass", lambda: eng.classwise_table(cw, N, nb, "mass", check=False)))
    for _, fn in arms:
        event_ms(fn, 3)                                                          # warm-up
    for name, fn in arms:
        ts = [event_ms(fn, a.launches) for _ in range(a.rounds)]
        print(json.dumps(dict(part="c", what="device time, HIP events, per call", arm=name, N=N, E=E, C=C, batch=B, n_bins=nb,
                              launches_per_timing=a.launches, timings=a.rounds, **stats(ts))), flush=True)
    for (o, _), m, yy in zip(cuts, means, ys):                                   # (one_cw rewrote batch 0 with itself: unchanged)
        eng.classwise_records(m, yy, cw, o)

    ed = width_edges(nb).astype(np.float64)

    def host_compute(pr):
        rows = np.concatenate([pr, np.cumsum(pr, axis=0) / np.arange(1, E + 1.0)[:, None, None]])
        pc = np.maximum(rows, 1e-256)
        conf = (pc / pc.sum(-1, keepdims=True)).astype(np.float32).astype(np.float64)              # [R, N, C]
        b = np.clip(np.searchsorted(ed, conf, side="left") - 1, 0, nb - 1)                          # bin 0 closed below
        flat = (np.arange(2 * E)[:, None, None] * C + np.arange(C)[None, None, :]) * nb + b
        hit = np.broadcast_to(np.arange(C)[None, None, :] == y[None, :, None], conf.shape)
        acc = np.bincount(flat.ravel(), weights=hit.ravel().astype(np.float64), minlength=2 * E * C * nb)
        cf = np.bincount(flat.ravel(), weights=conf.ravel(), minlength=2 * E * C * nb)
        return (np.abs(acc - cf).reshape(2 * E, C, nb).sum(-1) / N).mean(-1)

    copy_ms, compute_ms, val = [], [], None
    host_compute(preds.cpu().numpy())
    for _ in range(a.rounds):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        pr = preds.cpu().numpy()
        t1 = time.perf_counter()
        val = host_compute(pr)
        t2 = time.perf_counter()
        copy_ms.append((t1 - t0) * 1e3)
        compute_ms.append((t2 - t1) * 1e3)
    for name, ts in (("host route: mean.cpu(), 32 MB float64", copy_ms), ("host route: vectorised numpy classwise histogram", compute_ms)):
        print(json.dumps(dict(part="c", what="host clock", arm=name, N=N, E=E, C=C, n_bins=nb, timings=a.rounds, **stats(ts))), flush=True)
    ts = []
    for _ in range(a.rounds):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        dv = classwise_metrics(eng.classwise_table(cw, N, nb, "width"))["cw_ece"]
        ts.append((time.perf_counter() - t0) * 1e3)
    print(json.dumps(dict(part="c", what="host clock", arm="device route: classwise_table width + counters read + classwise_metrics", N=N,
                          timings=a.rounds, **stats(ts))), flush=True)
    print(json.dumps(dict(part="c", what="the two routes' classwise ECE", max_difference=float(np.abs(dv - val).max()),
                          device=[float(v) for v in dv])), flush=True)


def walk_ms(model, loader, rounds, arms, T=10):
    """Median host-clock milliseconds per batch of one ReliabilityAnalysis walk per arm (keyword sets), the arms alternating"""
    from bayesnn_fpga_amd.train import ReliabilityAnalysis
    times = {k: [] for k in arms}
    for kw in arms.values():
        ReliabilityAnalysis(model, loader, gpu=0, mc_passes=T, seed=0, **kw)      # warm-up: the engine, code objects
    for r in range(rounds):
        for k in (list(arms) if r % 2 == 0 else list(arms)[::-1]):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            ReliabilityAnalysis(model, loader, gpu=0, mc_passes=T, seed=0, **arms[k])
            torch.cuda.synchronize()
            times[k].append((time.perf_counter() - t0) * 1e3 / len(loader))
    return times


def part_w(a):
    from bayesnn_fpga_amd.synthetic import synthetic_images, synthetic_labels
    dev = torch.device("cuda", 0)
    model = model_of(SIZES["paper"][0], dev)
    B, nb = a.batch, 4
    x, y = synthetic_images(nb * B, seed=3), synthetic_labels(nb * B, a.classes, seed=4)
    loader = [(x[i * B:(i + 1) * B], y[i * B:(i + 1) * B]) for i in range(nb)]
    arms = {"classwise=False": {}, "classwise=True": dict(classwise=True), "classwise=False again": {}}
    for k, ts in walk_ms(model, loader, a.rounds, arms).items():
        print(json.dumps(dict(part="w", what="ReliabilityAnalysis walk, host clock, ms per batch", arm=k, batch=B, batches=nb, T=10,
                              timings=a.rounds, **stats(ts))), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--launches", type=int, default=20)
    ap.add_argument("--n", type=int, default=10000)
    ap.add_argument("--classes", type=int, default=100)
    ap.add_argument("--batch", type=int, default=250)
    ap.add_argument("--grid", type=int, default=2 ** 14)
    ap.add_argument("--parts", default="t")
    a = ap.parse_args()
    parts = a.parts.split(",")
    if set(parts) - {"r"} and not torch.cuda.is_available():
        sys.exit("reliability_bench.py measures parts t, k, c and w on the GPU: none visible (--parts r needs none)")
    for p in parts:
        {"r": part_r, "t": part_t, "k": part_k, "c": part_c, "w": part_w}[p](a)


if __name__ == "__main__":
    main()
