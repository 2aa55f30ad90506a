"""Fixed-T against adaptive Monte-Carlo sampling on the headline workload (ResNet-18 multi-exit, block + exit MC dropout, B = 250):
``predict(T=100)`` against ``predict_adaptive(T_max=100)`` at a few SEM thresholds, on the synthetic bench model and on its trained-like twin
(every classifier x 24, as bench.py's tolerance leg builds it), same process, alternating.  Prints one JSON line per measurement:
median wall time per batch, mean t_used, active_after_step and the largest |mean - mean at T = 100| over every exit, image and class.
Also: the cost of steps with no retirement against the same samples inside bmi_forward_mcd, a t_step sweep, and the device time of the
first site's MASK launches with and without a row table (bmi_profile_launches).

    python tools/adaptive_bench.py [--reps 5] [--quantiles 0.25,0.5,0.75] [--t-steps 10,20,25,50] [--dtype f16] [--ensemble]

--ensemble: per threshold also ``predict_adaptive(ensemble=True)`` (the exit-ensemble sums under the row table), alternating with the plain
call: its wall time with ``stop_on="exit"`` (the same steps: what the read-out costs) and with ``stop_on="ensemble"`` (the rule on the
ensemble of all exits at the SAME threshold), the mean t_used of both, and the device time of the ensemble.hip launches per step
(bmi_profile_launches, full-grid steps and image-list steps apart).

--votes: the decided-vote stop rule instead of the legs above (``predict_adaptive(ensemble=True, votes=True, rule="votes")``) against the
fixed-T ``predict_votes(T)``, alternating, on the headline model and on the exit-only C = 100 model (synthetic weights and the trained-like
twin of each), for slack 0, 1 and 2 and both ``stop_on``: mean t_used, wall time per batch, and the share of images whose ``vote_class`` at
the tested row equals the fixed run's — 1.0 at slack 0 by construction of the rule, asserted here.

The thresholds are the given quantiles of every image's SEM statistic after the first step (t = t_step) at the last exit, per model: a
fixed threshold that suits one set of weights retires nobody on the other.
"""
import argparse
import copy
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from bayesnn_fpga_amd.models.resnet18.resnet18 import ResNet18MCEarlyExit  # noqa: E402
from bayesnn_fpga_amd.synthetic import synthetic_images, synthetic_weights_  # noqa: E402

HEAD_NAMES = ("ex1linear", "ex2linear", "ex3linear", "linear")
KW = dict(dropout_exit=True, dropout="block", dropout_p=0.25, out_dim=10)


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    r = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, r


def mask_split(eng, fn, full_images):
    """Device ms and image-samples of the MASK-slot launches of one call, split into full-grid launches and row-table launches."""
    eng.profile(True)
    try:
        eng.profile_read()
        fn()
        torch.cuda.synchronize()
        eng.profile_read()
        launches = eng.profile_launches()
    finally:
        eng.profile(False)
    out = {"full": [0.0, 0], "rows": [0.0, 0]}
    for l in launches:
        if l["kind"] != "mask":
            continue
        k = "full" if l["images"] == full_images else "rows"
        out[k][0] += l["ms"]
        out[k][1] += l["images"]
    return {k: dict(ms=round(v[0], 4), images=v[1], us_per_1k_images=round(1e3 * v[0] / max(v[1], 1) * 1e3, 3)) for k, v in out.items()}


def ensemble_split(eng, fn, full_images):
    """Device ms of the ensemble.hip launches of one call: full-grid steps and image-list steps apart, per launch (= per step)."""
    eng.profile(True)
    try:
        eng.profile_read()
        fn()
        torch.cuda.synchronize()
        eng.profile_read()
        launches = [l for l in eng.profile_launches() if l["kind"] == "ensemble"]
    finally:
        eng.profile(False)
    out = {}
    for k, sel in (("full", lambda l: l["images"] == full_images), ("list", lambda l: l["images"] != full_images)):
        ms = [l["ms"] for l in launches if sel(l)]
        out[k] = dict(launches=len(ms), ms_per_step=round(float(np.mean(ms)), 4) if ms else None,
                      images=[l["images"] for l in launches if sel(l)])
    return out


def ensemble_leg(name, eng, x, a, t_step, thresholds):
    """predict_adaptive against predict_adaptive(ensemble=True), stop_on "exit" and "ensemble", alternating, at the leg's thresholds."""
    T = a.T
    calls = {
        "plain": lambda thr: eng.predict_adaptive(x, T, thr, t_step=t_step, seed=a.seed, uncertainty=True),
        "ensemble_stop_on_exit": lambda thr: eng.predict_adaptive(x, T, thr, t_step=t_step, seed=a.seed, ensemble=True),
        "ensemble_stop_on_ensemble": lambda thr: eng.predict_adaptive(x, T, thr, t_step=t_step, seed=a.seed, ensemble=True, stop_on="ensemble"),
    }
    for thr in thresholds:
        for fn in calls.values():
            fn(thr)                                                  # warm-up (the scratch is allocated here)
        times, res = {k: [] for k in calls}, {}
        for _ in range(a.reps):                                      # alternating, same process
            for k, fn in calls.items():
                ms, res[k] = timed(lambda: fn(thr))
                times[k].append(ms)
        med = {k: float(np.median(v)) for k, v in times.items()}
        steps = sum(1 for n in [x.shape[0]] + res["plain"]["active_after_step"][:-1] if n)
        prof = ensemble_split(eng, lambda: calls["ensemble_stop_on_exit"](thr), x.shape[0] * t_step)
        print(json.dumps(dict(model=name, what="adaptive_ensemble", rule="sem", threshold=thr, t_step=t_step, steps_run=steps,
                              ms={k: round(v, 3) for k, v in med.items()},
                              readout_ms_per_step=round((med["ensemble_stop_on_exit"] - med["plain"]) / max(steps, 1), 4),
                              ensemble_kernel=prof,
                              mean_t_used={k: round(float(r["t_used"].float().mean()), 2) for k, r in res.items()},
                              active_after_step={k: r["active_after_step"] for k, r in res.items()})), flush=True)


def votes_leg(name, model, dev, x, a):
    """predict_votes(T) against predict_adaptive(rule="votes") at slack 0, 1, 2, stop_on "exit" and "ensemble", alternating."""
    B, T = x.shape[0], a.T
    eng = model.engine(dev, max_batch=B, dtype=a.dtype)
    t_step = min(a.t_step, eng.chunk_samples)
    calls = {"fixed": lambda: eng.predict_votes(x, T, seed=a.seed)}
    for stop_on in ("exit", "ensemble"):
        for slack in (0, 1, 2):
            calls[stop_on, slack] = (lambda so=stop_on, sl=slack: eng.predict_adaptive(x, T, sl, rule="votes", t_step=t_step, seed=a.seed,
                                                                                       ensemble=True, stop_on=so, votes=True))
    for fn in calls.values():                                        # warm-up of every path (the scratch is allocated here)
        fn()
    times, res = {k: [] for k in calls}, {}
    for _ in range(a.reps):                                          # alternating, same process
        for k, fn in calls.items():
            ms, res[k] = timed(fn)
            times[k].append(ms)
    fixed = float(np.median(times["fixed"]))
    print(json.dumps(dict(model=name, what="fixed_votes", T=T, B=B, dtype=a.dtype, t_step=t_step, ms=round(fixed, 3),
                          mean_variation_ratio_last_exit=round(float(res["fixed"]["variation_ratio"][-1].mean()), 4))), flush=True)
    for k, r in res.items():
        if k == "fixed":
            continue
        stop_on, slack = k
        key = "vote_class" if stop_on == "exit" else "ens_vote_class"
        same = float((r[key][-1] == res["fixed"][key][-1]).float().mean())
        if slack == 0:
            assert same == 1.0, f"slack 0 must keep the full run's majority vote ({name}, stop_on={stop_on}: {same})"
        ms = float(np.median(times[k]))
        steps = sum(1 for n in [B] + r["active_after_step"][:-1] if n)
        print(json.dumps(dict(model=name, what="adaptive_votes", stop_on=stop_on, slack=slack, t_step=t_step, ms=round(ms, 3),
                              vs_fixed=round(ms / fixed, 3), ms_per_step=round(ms / max(steps, 1), 3), steps_run=steps,
                              mean_t_used=round(float(r["t_used"].float().mean()), 2),
                              work_fraction=round(float(r["t_used"].float().mean()) / T, 3), active_after_step=r["active_after_step"],
                              same_vote_class_as_fixed=same)), flush=True)
    model.invalidate_engine()


def twin_of(model):
    """The trained-like twin: every classifier x 24, as bench.py's tolerance leg builds it"""
    twin = copy.deepcopy(model)
    with torch.no_grad():
        for n in HEAD_NAMES:
            getattr(twin, n).weight.mul_(24.0)
    twin.invalidate_engine()
    return twin


def leg(name, model, dev, x, a):
    B, T = x.shape[0], a.T
    eng = model.engine(dev, max_batch=B, dtype=a.dtype)
    t_step = min(a.t_step, eng.chunk_samples)
    S = eng.new_moments(B)
    eng.accumulate(x, S, 0, t_step, a.seed)
    m = S[0, -1] / t_step
    sem = ((S[1, -1] / t_step - m * m).clamp_min(0) / t_step).sqrt().max(-1).values
    thresholds = [float(torch.quantile(sem, float(q))) for q in a.quantiles.split(",")]
    ref = eng.predict(x, T, seed=a.seed)["mean"]
    for _ in range(2):                                               # warm-up of every path
        eng.predict(x, T, seed=a.seed)
        for thr in thresholds:
            eng.predict_adaptive(x, T, thr, t_step=t_step, seed=a.seed)
    times = {"fixed": []}
    res = {}
    for _ in range(a.reps):                                          # alternating, same process
        times["fixed"].append(timed(lambda: eng.predict(x, T, seed=a.seed))[0])
        for thr in thresholds:
            ms, r = timed(lambda: eng.predict_adaptive(x, T, thr, t_step=t_step, seed=a.seed))
            times.setdefault(thr, []).append(ms)
            res[thr] = r
    fixed = float(np.median(times["fixed"]))
    print(json.dumps(dict(model=name, what="fixed", T=T, B=B, dtype=a.dtype, ms=round(fixed, 3))))
    for thr in thresholds:
        r = res[thr]
        ms = float(np.median(times[thr]))
        print(json.dumps(dict(model=name, what="adaptive", rule="sem", threshold=thr, t_step=t_step, ms=round(ms, 3),
                              vs_fixed=round(ms / fixed, 3), mean_t_used=round(float(r["t_used"].float().mean()), 2),
                              work_fraction=round(float(r["t_used"].float().mean()) / T, 3), active_after_step=r["active_after_step"],
                              max_abs_dmean_vs_T_tested_exit=float((r["mean"][-1] - ref[-1]).abs().max()),
                              max_abs_dmean_vs_T_any_exit=float((r["mean"] - ref).abs().max()))))
    # steps with no retirement (threshold -1: the SEM is never <= -1) against the same samples inside bmi_forward_mcd
    for steps in (1, T // t_step):
        Tn = steps * t_step
        tf, ta = [], []
        for _ in range(a.reps):
            tf.append(timed(lambda: eng.predict(x, Tn, seed=a.seed))[0])
            ta.append(timed(lambda: eng.predict_adaptive(x, Tn, -1.0, t_step=t_step, seed=a.seed))[0])
        print(json.dumps(dict(model=name, what="no_retirement", steps=steps, samples=Tn, fixed_ms=round(float(np.median(tf)), 3),
                              adaptive_ms=round(float(np.median(ta)), 3),
                              per_step_overhead_ms=round((float(np.median(ta)) - float(np.median(tf))) / steps, 3))))
    return eng, t_step, thresholds


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=250)
    ap.add_argument("--T", type=int, default=100)
    ap.add_argument("--t-step", type=int, default=25)
    ap.add_argument("--t-steps", default="10,20,25,50")
    ap.add_argument("--quantiles", default="0.25,0.5,0.75")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--seed", type=int, default=3)
    ap.add_argument("--dtype", default="f16")
    ap.add_argument("--ensemble", action="store_true", help="also measure predict_adaptive(ensemble=True) at the same thresholds")
    ap.add_argument("--votes", action="store_true", help="measure the decided-vote stop rule against predict_votes, and nothing else")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    if a.votes:
        x = synthetic_images(a.batch, seed=1234).to(dev)
        for tag, kw in (("headline_c10", KW), ("exit_only_c100", dict(dropout_exit=True, dropout=None, dropout_p=0.25, out_dim=100))):
            torch.manual_seed(0)
            model = synthetic_weights_(ResNet18MCEarlyExit(**kw), 0).to(dev).eval()
            votes_leg(tag + "/synthetic", model, dev, x, a)
            votes_leg(tag + "/trained_like_twin", twin_of(model), dev, x, a)
        return
    model = synthetic_weights_(ResNet18MCEarlyExit(**KW), 0).to(dev).eval()
    x = synthetic_images(a.batch, seed=1234).to(dev)
    twin = twin_of(model)
    for name, m in (("synthetic", model), ("trained_like_twin", twin)):
        eng, t_step, thresholds = leg(name, m, dev, x, a)
        if a.ensemble:
            ensemble_leg(name, eng, x, a, t_step, thresholds)
        if name == "synthetic":
            thr = thresholds[len(thresholds) // 2]
            print(json.dumps(dict(model=name, what="mask_launches", threshold=thr, t_step=t_step,
                                  **mask_split(eng, lambda: eng.predict_adaptive(x, a.T, thr, t_step=t_step, seed=a.seed), a.batch * t_step))))
            for ts in (int(v) for v in a.t_steps.split(",")):
                ts = min(ts, eng.chunk_samples)
                ms = []
                for _ in range(a.reps):
                    t, r = timed(lambda: eng.predict_adaptive(x, a.T, thr, t_step=ts, seed=a.seed))
                    ms.append(t)
                print(json.dumps(dict(model=name, what="t_step_sweep", threshold=thr, t_step=ts, ms=round(float(np.median(ms)), 3),
                                      mean_t_used=round(float(r["t_used"].float().mean()), 2), active_after_step=r["active_after_step"])))
        m.invalidate_engine()


if __name__ == "__main__":
    main()
