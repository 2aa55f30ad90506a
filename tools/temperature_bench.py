#!/usr/bin/env python3
"""Temperature scaling, measured (same process, alternating A/B in the style of tools/step_ab.py).  One JSON line per measurement.

  (a) the headline step (ResNet-18 block + exit dropout, B = 250, T = 100) and the exit-only step (C = 100, T = 10) with the temperature
      off against tau = 2: whole-step medians with the spread of each arm (min .. max over the rounds), and the head launches' time from
      the engine's profiler (bmi_profile_*) in a run of their own;
  (b) one nll_grid launch (B = 250, T = 10, C = 100, E = 4, G = 33) and one full fit — the walk that produces the logits plus the
      search rounds — for N = 10 000, set against the forward walk alone; work counted from the shapes;
  (c) the trained-like twin (classifiers x 24) with teacher labels drawn at tau* = 3 from the final exit: NLL and hist-ECE per exit before
      and after the fit, and the exit histogram of predict_early_exit at confidence 0.9 before and after.

    python tools/temperature_bench.py [--rounds 9] [--steps 3] [--n 10000] [--parts a,b,c]
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from bayesnn_fpga_amd.models.resnet18.resnet18 import ResNet18MCEarlyExit  # noqa: E402
from bayesnn_fpga_amd.synthetic import synthetic_images, synthetic_weights_  # noqa: E402
from bayesnn_fpga_amd.train.calibration import TemperatureScaling, temper_logits  # noqa: E402
from bayesnn_fpga_amd.train.metrics import ece_hist_binary  # noqa: E402

HEADLINE = (dict(dropout_exit=True, dropout="block", dropout_p=0.25, out_dim=10), 250, 100)
EXIT_ONLY = (dict(dropout_exit=True, dropout=None, dropout_p=0.25, out_dim=100), 250, 10)
HEADS = ("ex1linear", "ex2linear", "ex3linear", "linear")
DEV = torch.device("cuda", 0)


def model_of(kw, gain=None):
    torch.manual_seed(0)
    np.random.seed(0)
    m = synthetic_weights_(ResNet18MCEarlyExit(**kw), 0)
    if gain:
        with torch.no_grad():
            for n in HEADS:
                getattr(m, n).weight.mul_(gain)
    return m.to(DEV).eval()


def timed_ms(fn, steps):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / steps * 1e3


def part_a(a):
    for name, (kw, B, T) in (("headline", HEADLINE), ("exit_only", EXIT_ONLY)):
        eng = model_of(kw).engine(DEV, max_batch=B, dtype="f16")
        x = synthetic_images(B, seed=1234).to(DEV)
        S = eng.new_moments(B)

        def step():
            S.zero_()
            eng.accumulate(x, S, 0, T, 42)
            return eng.finalize(S, T)
        arms = {"off": None, "tau_2": 2.0}
        times = {k: [] for k in arms}
        for tau in arms.values():                     # warm both instantiations
            eng.set_temperature(tau)
            step(), step()
        for _ in range(a.rounds):                     # alternating
            for k, tau in arms.items():
                eng.set_temperature(tau)
                times[k].append(timed_ms(step, a.steps))
        heads = {}
        for k, tau in arms.items():                   # the profiler's event records slow the host: a run of its own
            eng.set_temperature(tau)
            eng.profile(True)
            eng.profile_read()
            step()
            torch.cuda.synchronize()
            prof = eng.profile_read()
            eng.profile(False)
            heads[k] = dict(ms=round(prof["head"][0], 4), launches=int(prof["head"][1]))
        out = dict(part="a", workload=name, B=B, T=T, rounds=a.rounds, steps=a.steps)
        for k in arms:
            t = sorted(times[k])
            out[k] = dict(median_ms=round(t[len(t) // 2], 4), min_ms=round(t[0], 4), max_ms=round(t[-1], 4), head=heads[k])
        out["median_ratio_tau_over_off"] = round(out["tau_2"]["median_ms"] / out["off"]["median_ms"], 4)
        print(json.dumps(out), flush=True)
        eng.set_temperature(None)


def part_b(a):
    kw, B, T = EXIT_ONLY
    C, E, G = kw["out_dim"], 4, 33
    m = model_of(kw)
    eng = m.engine(DEV, max_batch=B, dtype="f16")
    x = synthetic_images(B, seed=1234).to(DEV)
    logits = eng.forward_samples(x, T, seed=1)
    y = torch.randint(0, C, (B,), generator=torch.Generator().manual_seed(0)).to(DEV)
    tau = torch.from_numpy(np.stack([np.exp(np.linspace(np.log(0.05), np.log(20.0), G))] * E).astype(np.float32)).to(DEV)
    out = torch.zeros(E, G, dtype=torch.float64, device=DEV)
    launch = lambda: eng.nll_grid(logits, y, tau, out=out)           # noqa: E731
    fwd = lambda: eng.forward_samples(x, T, seed=1, out=logits)      # noqa: E731
    launch(), fwd()
    t_nll = sorted(timed_ms(launch, 20) for _ in range(a.rounds))
    t_fwd = sorted(timed_ms(fwd, 20) for _ in range(a.rounds))
    exps = B * E * T * G * C
    med = t_nll[len(t_nll) // 2]
    print(json.dumps(dict(part="b", what="nll_grid launch", B=B, T=T, C=C, E=E, G=G, median_ms=round(med, 4), min_ms=round(t_nll[0], 4),
                          max_ms=round(t_nll[-1], 4), float64_exps=exps, gexp_per_s=round(exps / med / 1e6, 2),
                          logit_bytes=int(logits.numel() * 4), gb_per_s=round(logits.numel() * 4 / med / 1e6, 2),
                          forward_samples_median_ms=round(t_fwd[len(t_fwd) // 2], 4))), flush=True)
    # the whole fit: N images in batches of B
    N = a.n
    xs = synthetic_images(N, seed=77)
    ys = torch.randint(0, C, (N,), generator=torch.Generator().manual_seed(1))
    loader = [(xs[i:i + B], ys[i:i + B]) for i in range(0, N, B)]
    m.engine_dtype = "f16"
    ts = TemperatureScaling(m, loader, gpu=0, mc_passes=T, seed=0)
    ts.fit()                                                          # warm
    t_walk, t_fit = [], []
    for _ in range(3):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        ts.collect()
        torch.cuda.synchronize()
        t_walk.append((time.perf_counter() - t0) * 1e3)
        t0 = time.perf_counter()
        r = ts.fit()
        torch.cuda.synchronize()
        t_fit.append((time.perf_counter() - t0) * 1e3)
    print(json.dumps(dict(part="b", what="full fit", N=N, batches=len(loader), T=T, C=C, E=E, rounds=int(r["rounds"]),
                          walk_ms=round(float(np.median(t_walk)), 2), walk_plus_search_ms=round(float(np.median(t_fit)), 2),
                          search_ms=round(float(np.median(t_fit) - np.median(t_walk)), 2),
                          nll_launches=int(r["rounds"]) * len(loader))), flush=True)


def part_c(a):
    kw = dict(dropout_exit=True, dropout="block", dropout_p=0.25, out_dim=10)
    sizes, T, seed, C = [1000, 1000, 1000, 600], 10, 5, 10
    m = model_of(kw, gain=24.0)
    m.engine_dtype = "f16x2"
    x = synthetic_images(sum(sizes), seed=31)
    offs = np.concatenate([[0], np.cumsum(sizes)])
    eng = m.engine(DEV, max_batch=max(sizes))
    raw = np.concatenate([eng.forward_samples(x[offs[k]:offs[k + 1]].to(DEV), T, seed=seed + k).cpu().numpy() for k in range(len(sizes))], axis=2)
    rng = np.random.default_rng(7)
    labels = np.array([rng.choice(C, p=q / q.sum()) for q in temper_logits(raw, 3.0)[0][-1]])
    y = torch.from_numpy(labels)
    loader = [(x[offs[k]:offs[k + 1]], y[offs[k]:offs[k + 1]]) for k in range(len(sizes))]
    ts = TemperatureScaling(m, loader, gpu=0, mc_passes=T, seed=seed)
    r = ts.fit()
    onehot = np.eye(C)[labels]
    xb = x[:250].to(DEV)

    def state():
        mean, _ = temper_logits(raw, m.exit_temperature or 1.0)
        e = m.engine(DEV, max_batch=max(sizes))
        hist = np.bincount(e.predict_early_exit(xb, T, 0.9, seed=seed)["exit_layer"].cpu().numpy(), minlength=4).tolist()
        return dict(hist_ece=[round(ece_hist_binary(mean[k], onehot), 5) for k in range(4)], exit_hist_at_0p9=hist)
    before = state()
    ts.apply()
    after = state()
    print(json.dumps(dict(part="c", n=int(r["n"]), tau=[round(float(t), 5) for t in r["tau"]], at_bound=[bool(b) for b in r["at_bound"]],
                          rounds=int(r["rounds"]), nll_before=[round(float(v), 3) for v in r["nll_before"]],
                          nll_after=[round(float(v), 3) for v in r["nll_after"]], before=before, after=after)), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--n", type=int, default=10000)
    ap.add_argument("--parts", default="a,b,c")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("temperature_bench.py measures on the GPU: none visible")
    for p in a.parts.split(","):
        {"a": part_a, "b": part_b, "c": part_c}[p](a)


if __name__ == "__main__":
    main()
