"""Full ``predict`` against early exit by stages (``predict_early_exit``), same process, alternating, on the exit workloads: ResNet-18
exit-only dropout (C = 100, T = 10), VGG-19 exit-only (C = 100, T = 10) and the headline ResNet-18 block + exit (T = 20), at B = 250 and,
where the engine plans it, B = 1024.  Thresholds: the confidence statistic's quantiles at exit 1 on the full run, so that about 25 / 50 / 75 %
of the images leave there.  Prints one JSON line per measurement: median ms of both calls, exit histogram, macs_done / macs_full, and per
stage the images each launch carried (bmi_profile_launches).

    python tools/exit_bench.py [--reps 7] [--batches 250,1024] [--leave 0.25,0.5,0.75] [--dtype f16] [--ensemble]

--ensemble: also ``predict_early_exit(ensemble_readout=True)`` (the exit-ensemble sums of the exits every image reached: the heads leave
their logits in the scratch, one ensemble.hip launch behind the last stage that ran), alternating with the two other calls: its median ms,
the difference per stage that ran, and the device time of that one launch (bmi_profile_launches).
"""
import argparse
import collections
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from bayesnn_fpga_amd.models.resnet18.resnet18 import ResNet18MCEarlyExit  # noqa: E402
from bayesnn_fpga_amd.models.vgg19.vgg19 import VGG19MCEarlyExit  # noqa: E402
from bayesnn_fpga_amd.synthetic import synthetic_images, synthetic_weights_  # noqa: E402

EXIT_ONLY = dict(dropout_exit=True, dropout=None, dropout_p=0.25, out_dim=100)
WORKLOADS = {
    "resnet18_exit_only": (ResNet18MCEarlyExit, EXIT_ONLY, 10),
    "vgg19_me": (VGG19MCEarlyExit, EXIT_ONLY, 10),
    "resnet18_me": (ResNet18MCEarlyExit, dict(dropout_exit=True, dropout="block", dropout_p=0.25, out_dim=10), 20),
}


def median_ms(fn, reps):
    out = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        out.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(out))


def launch_images(eng, fn):
    """Counter of the images carried by each launch of one call."""
    eng.profile(True)
    try:
        eng.profile_read()
        fn()
        torch.cuda.synchronize()
        eng.profile_read()
        launches = eng.profile_launches()
    finally:
        eng.profile(False)
    return dict(sorted(collections.Counter(ln["images"] for ln in launches).items()))


def ensemble_launch_ms(eng, fn):
    """Device ms of the ensemble.hip launch of one call (the exit-count fill included)."""
    eng.profile(True)
    try:
        eng.profile_read()
        fn()
        torch.cuda.synchronize()
        eng.profile_read()
        ms = [ln["ms"] for ln in eng.profile_launches() if ln["kind"] == "ensemble"]
    finally:
        eng.profile(False)
    return round(float(sum(ms)), 4), len(ms)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--batches", default="250,1024")
    ap.add_argument("--leave", default="0.25,0.5,0.75")
    ap.add_argument("--dtype", default="f16")
    ap.add_argument("--workloads", default=",".join(WORKLOADS))
    ap.add_argument("--ensemble", action="store_true", help="also measure predict_early_exit(ensemble_readout=True)")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    for name in a.workloads.split(","):
        cls, kw, T = WORKLOADS[name]
        for B in (int(b) for b in a.batches.split(",")):
            torch.manual_seed(0)
            m = synthetic_weights_(cls(**kw), 0).to(dev).eval()
            try:
                eng = m.engine(dev, max_batch=B, chunk_samples=T, dtype=a.dtype)
            except Exception as ex:      # (an engine the planner refuses at this batch)
                print(json.dumps(dict(workload=name, B=B, skipped=str(ex))), flush=True)
                continue
            x = synthetic_images(B, seed=1).to(dev)
            full = eng.predict(x, T, seed=3)
            conf1 = full["mean"][1].max(-1).values.cpu().numpy()
            for frac in (float(f) for f in a.leave.split(",")):
                thr = float(np.quantile(conf1, 1.0 - frac))
                ee = lambda: eng.predict_early_exit(x, T, thr, seed=3)       # noqa: E731
                pr = lambda: eng.predict(x, T, seed=3)                      # noqa: E731
                eu = lambda: eng.predict_early_exit(x, T, thr, seed=3, uncertainty=True)            # noqa: E731
                er = lambda: eng.predict_early_exit(x, T, thr, seed=3, ensemble_readout=True)       # noqa: E731
                ee(), pr()
                if a.ensemble:
                    eu(), er()
                ms_full, ms_exit, ms_unc, ms_read = [], [], [], []
                for _ in range(a.reps):           # alternating
                    ms_full.append(median_ms(pr, 1))
                    ms_exit.append(median_ms(ee, 1))
                    if a.ensemble:
                        ms_unc.append(median_ms(eu, 1))
                        ms_read.append(median_ms(er, 1))
                r = ee()
                extra = {}
                if a.ensemble:
                    stages = 1 + sum(1 for n in r["active_after"][1:-1] if n)
                    k_ms, k_n = ensemble_launch_ms(eng, er)
                    extra = dict(ms_early_exit_uncertainty=round(float(np.median(ms_unc)), 4),
                                 ms_early_exit_readout=round(float(np.median(ms_read)), 4), stages_run=stages,
                                 readout_ms_per_stage=round((float(np.median(ms_read)) - float(np.median(ms_unc))) / stages, 4),
                                 ensemble_launches=k_n, ensemble_launch_ms=k_ms)
                hist = np.bincount(r["exit_layer"].cpu().numpy(), minlength=eng.n_exits).tolist()
                print(json.dumps(dict(workload=name, dtype=a.dtype, B=B, T=T, leave_at_exit1=frac, threshold=round(thr, 6), exit_hist=hist,
                                      active_after=r["active_after"], ms_predict=round(float(np.median(ms_full)), 4),
                                      ms_early_exit=round(float(np.median(ms_exit)), 4), macs_ratio=round(r["macs_done"] / r["macs_full"], 4),
                                      launch_images=launch_images(eng, ee), **extra)), flush=True)
            del eng, m
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
