#!/usr/bin/env python3
"""The joint temperature fit of the exit ensembles, measured.  One JSON line per measurement.

  (a) one coordinate-step launch of ensemble_nll_grid (B = 250, T = 10, E = 4, C = 100, G = 33; one exit varied), one shared-temperature
      launch (every exit varied) and one nll_grid launch on the same logits: HIP-event medians after a warm-up, each timing a run of
      launches between two events; and one full fit for N = 10 000 (40 batches of 250): the walk, the per-exit fit and the joint search;
  (b) on the trained-like twin (classifiers x 24) and on the plain synthetic model, block + exit and exit-only dropout, C in {10, 100},
      teacher labels drawn at tau* = 3 from the final exit (as tests/test_temperature.py draws them): NLL and hist-ECE of the full
      ensemble (row E - 1) at tau = 1, at the per-exit fit, and at the joint fit ("vector" and "shared"), with the number of sweeps.

    python tools/ensemble_temperature_bench.py [--rounds 9] [--launches 20] [--n 10000] [--parts a,b]
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
from bayesnn_fpga_amd.train.calibration import EnsembleTemperatureScaling, temper_logits  # noqa: E402
from bayesnn_fpga_amd.train.metrics import ece_hist_binary  # noqa: E402

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


def event_ms(fn, launches):
    """HIP-event time of ``launches`` back-to-back calls, per call."""
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


def part_a(a):
    kw, B, T = dict(dropout_exit=True, dropout=None, dropout_p=0.25, out_dim=100), 250, 10
    C, E, G = kw["out_dim"], 4, 33
    m = model_of(kw)
    eng = m.engine(DEV, max_batch=B, dtype="f16")
    x = synthetic_images(B, seed=1234).to(DEV)
    logits = eng.forward_samples(x, T, seed=1)
    y = torch.randint(0, C, (B,), generator=torch.Generator().manual_seed(0)).to(DEV)
    cand = torch.from_numpy(np.exp(np.linspace(np.log(0.05), np.log(20.0), G)).astype(np.float32)).to(DEV)
    grid = cand[None].repeat(E, 1).contiguous()
    out = torch.zeros(E, G, dtype=torch.float64, device=DEV)
    # straight through the C ABI on buffers made once: the Python wrappers' checks and the upload of tau are not the launch
    lib, ones = eng.lib, torch.ones(E, device=DEV)
    y32 = y.to(torch.int32)
    scratch = torch.empty(lib.bmi_nll_ensemble_temperature_scratch_bytes(E, B, G), dtype=torch.uint8, device=DEV)
    stream = eng._stream()

    def per_exit():
        return lib.bmi_nll_temperature_grid(logits.data_ptr(), T, E, B, C, y32.data_ptr(), grid.data_ptr(), G, out.data_ptr(), scratch.data_ptr(),
                                            scratch.numel(), stream)

    def joint(mask):
        return lambda: lib.bmi_nll_ensemble_temperature_grid(logits.data_ptr(), T, E, B, C, y32.data_ptr(), ones.data_ptr(), mask, cand.data_ptr(), G,
                                                             out.data_ptr(), scratch.data_ptr(), scratch.numel(), stream)
    arms = {"nll_grid (per-exit, all E)": per_exit, "ensemble_nll_grid, exit 0 varied": joint(1), "ensemble_nll_grid, exit 3 varied": joint(8),
            "ensemble_nll_grid, all exits varied": joint(15),
            "ensemble_nll_grid, exit 3 varied, through MCDEngine": lambda: eng.ensemble_nll_grid(logits, y, 1.0, 3, cand, out=out)}
    assert per_exit() == 0 and joint(8)() == 0
    times = {k: [] for k in arms}
    for fn in arms.values():                          # warm
        for _ in range(5):
            fn()
    torch.cuda.synchronize()
    for _ in range(a.rounds):                         # alternating
        for k, fn in arms.items():
            times[k].append(event_ms(fn, a.launches))
    exps = {"nll_grid (per-exit, all E)": B * T * E * G * C, "ensemble_nll_grid, all exits varied": B * T * E * G * C}
    for k in arms:
        d = dict(part="a", what=k, B=B, T=T, C=C, E=E, G=G, launches_per_timing=a.launches, timings=a.rounds, **stats(times[k]))
        d["float64_exps"] = exps.get(k, B * T * C * (6 * (E - 1) + G))      # six candidate slices restate the fixed exits
        print(json.dumps(d), flush=True)
    # the whole fit: N images in batches of B
    N = a.n
    xs = synthetic_images(N, seed=77)
    ys = torch.randint(0, C, (N,), generator=torch.Generator().manual_seed(1))
    loader = [(xs[i:i + B], ys[i:i + B]) for i in range(0, N, B)]
    m.engine_dtype = "f16"
    ets = EnsembleTemperatureScaling(m, loader, gpu=0, mc_passes=T, seed=0)
    for mode, init in (("vector", "per_exit"), ("vector", "ones"), ("shared", "ones")):
        ets.fit(mode=mode, init=init)                 # warm
        t_walk, t_fit = [], []
        for _ in range(3):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            ets.collect()
            torch.cuda.synchronize()
            t_walk.append((time.perf_counter() - t0) * 1e3)
            t0 = time.perf_counter()
            r = ets.fit(mode=mode, init=init)
            torch.cuda.synchronize()
            t_fit.append((time.perf_counter() - t0) * 1e3)
        print(json.dumps(dict(part="a", what="full fit", mode=mode, init=init, N=N, batches=len(loader), T=T, C=C, E=E, sweeps=int(r["sweeps"]),
                              stopped_by_rule=bool(r["stopped_by_rule"]), walk_ms=round(float(np.median(t_walk)), 2),
                              walk_plus_fit_ms=round(float(np.median(t_fit)), 2),
                              fit_ms=round(float(np.median(t_fit) - np.median(t_walk)), 2))), flush=True)


def part_b(a):
    sizes, T, seed = [1000, 1000, 1000, 600], 10, 5
    x = synthetic_images(sum(sizes), seed=31)
    offs = np.concatenate([[0], np.cumsum(sizes)])
    for gain in (24.0, None):
        for dropout in ("block", None):
            for C in (10, 100):
                kw = dict(dropout_exit=True, dropout=dropout, dropout_p=0.25, out_dim=C)
                m = model_of(kw, gain=gain)
                m.engine_dtype = "f16x2"
                eng = m.engine(DEV, max_batch=max(sizes))
                raw = np.concatenate([eng.forward_samples(x[offs[k]:offs[k + 1]].to(DEV), T, seed=seed + k).cpu().numpy()
                                      for k in range(len(sizes))], axis=2)
                rng = np.random.default_rng(7)
                labels = np.array([rng.choice(C, p=q / q.sum()) for q in temper_logits(raw, 3.0)[0][-1]])
                y = torch.from_numpy(labels)
                loader = [(x[offs[k]:offs[k + 1]], y[offs[k]:offs[k + 1]]) for k in range(len(sizes))]
                onehot = np.eye(C)[labels]

                def ece(tau):
                    return round(float(ece_hist_binary(temper_logits(raw, tau)[0].mean(0), onehot)), 5)
                ets = EnsembleTemperatureScaling(m, loader, gpu=0, mc_passes=T, seed=seed)
                rv = ets.fit(mode="vector", init="per_exit")
                rs = ets.fit(mode="shared", init="ones")
                rd = lambda v: [round(float(t), 4) for t in v]       # noqa: E731
                print(json.dumps(dict(
                    part="b", model="x24 twin" if gain else "plain", dropout="block + exit" if dropout else "exit-only", C=C, n=int(rv["n"]),
                    ones=dict(nll=round(float(rv["nll_ones"][-1]), 3), ece=ece(1.0)),
                    per_exit=dict(tau=rd(rv["tau_init"]), nll=round(float(rv["nll_per_exit"][-1]), 3), ece=ece(rv["tau_init"])),
                    vector=dict(tau=rd(rv["tau"]), nll=round(float(rv["nll_after"][-1]), 3), ece=ece(rv["tau"]), sweeps=int(rv["sweeps"]),
                                stopped_by_rule=bool(rv["stopped_by_rule"]), at_bound=[bool(b) for b in rv["at_bound"]]),
                    shared=dict(tau=rd(rs["tau"]), nll=round(float(rs["nll_after"][-1]), 3), ece=ece(rs["tau"]), sweeps=int(rs["sweeps"]),
                                at_bound=[bool(b) for b in rs["at_bound"]]))), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--launches", type=int, default=20)
    ap.add_argument("--n", type=int, default=10000)
    ap.add_argument("--parts", default="a,b")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("ensemble_temperature_bench.py measures on the GPU: none visible")
    for p in a.parts.split(","):
        {"a": part_a, "b": part_b}[p](a)


if __name__ == "__main__":
    main()
