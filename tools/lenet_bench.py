"""BASELINE config 1 on the device: MC-dropout LeNet-5, T = 10, device-resident input to final mean and variance
(``LeNet5Engine.predict``), beside the oracle's ``mcd_predict`` on the host CPU.  Prints one JSON line per (num_bayes_layer, batch), then
one per batch for the multi-exit model ``LeNet5MCEarlyExit`` (model = "lenet5_me": both exits' moments from one launch).

    python tools/lenet_bench.py [--iters 30] [--warmup 5] [--cpu-iters 3]

``--early-exit``: instead, the multi-exit model at B = 1024, T = 100: ``predict`` beside ``predict_early_exit`` (confidence rule) at three
thresholds taken from that batch's own early-exit statistics, so that none, about half and all of the images leave.  The four calls
alternate inside every iteration; one JSON line each.

    python tools/lenet_bench.py --early-exit [--batch 1024] [--iters 30] [--warmup 5]

``--masks M``: instead, the Masksembles model (``mask_type="mask"``, M masks: csrc/lenet5_mask.hip) beside the MC-dropout model at the same
(num_bayes_layer, B, T): k = 3 at B = 1024 and 250 with T = M and T = 100, k = 1 at B = 1024 with T = M.  The two calls alternate inside every
iteration; one JSON line each.

    python tools/lenet_bench.py --masks 4 [--iters 30] [--warmup 5]

``--quant W,I``: instead, the quantised model (``quant_tbit=W, quant_ibit=I``: csrc/qlenet5.hip) beside the fp16 model at the same
(num_bayes_layer, B, T): k = 1 and 3, B = 250 and 1024, T = 10 and 100; then the multi-exit pair, quantised ``LeNet5MCEarlyExit``
(csrc/qlenet5_me.hip) beside the fp16 one, at B = 250 and 1024, T = 3, 10 and 100.  The two calls alternate inside every iteration; one JSON
line each.

    python tools/lenet_bench.py --quant 6,0 [--iters 30] [--warmup 5]
"""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

from bayesnn_fpga_amd.models import extra as bx  # noqa: E402
from bayesnn_fpga_amd.synthetic import synthetic_images, synthetic_weights_  # noqa: E402
from oracle import extra_models as ox  # noqa: E402
from oracle import mcd  # noqa: E402


def early_exit(a, dev, T=100):
    B = a.batch
    torch.manual_seed(0)
    m = synthetic_weights_(bx.LeNet5MCEarlyExit(dropout_p=0.25), 0).to(dev).eval()
    x = synthetic_images(B, 1234, channels=1, size=28).to(dev)
    eng = m.engine(dev, max_batch=B)
    stat = eng.predict(x, T, seed=1)["mean"][0].max(dim=1).values.cpu()
    calls = [("predict", None)] + [(f"predict_early_exit, {name} leave", float(thr)) for name, thr in
                                   (("none", stat.max()), ("half", stat.median()), ("all", stat.min() - 1e-6))]
    run = lambda thr: eng.predict(x, T, seed=1) if thr is None else eng.predict_early_exit(x, T, thr, seed=1)
    us, last = {name: [] for name, _ in calls}, {}
    for it in range(a.warmup + a.iters):
        for name, thr in calls:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            r = run(thr)
            e1.record()
            e1.synchronize()
            if it >= a.warmup:
                us[name].append(e0.elapsed_time(e1) * 1e3)
            last[name] = r
    for name, thr in calls:
        med = statistics.median(us[name])
        row = dict(model=m.family, call=name, batch=B, T=T, us_per_call=round(med, 1), us_min=round(min(us[name]), 1), us_max=round(max(us[name]), 1),
                   iters=a.iters, device=torch.cuda.get_device_name(0))
        if thr is not None:
            r = last[name]
            row.update(threshold=thr, images_left=B - r["active_after"][0], macs_done_over_full=round(r["macs_done"] / r["macs_full"], 4))
        print(json.dumps(row), flush=True)


def masksembles(a, dev):
    M = a.masks
    for k, B, T in ((3, 1024, M), (3, 250, M), (3, 1024, 100), (3, 250, 100), (1, 1024, M)):
        x = synthetic_images(B, 1234, channels=1, size=28).to(dev)
        engines = {}
        for name, kw in (("mc", {}), ("mask", dict(mask_type="mask", num_masks=M))):
            torch.manual_seed(0)
            m = synthetic_weights_(bx.LeNet5MC(num_bayes_layer=k, dropout_p=0.25, **kw), 0).to(dev).eval()
            engines[name] = (m, m.engine(dev, max_batch=B))
        us = {name: [] for name in engines}
        for it in range(a.warmup + a.iters):
            for name, (_, eng) in engines.items():
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                eng.predict(x, T, seed=1)
                e1.record()
                e1.synchronize()
                if it >= a.warmup:
                    us[name].append(e0.elapsed_time(e1) * 1e3)
        for name in engines:
            med = statistics.median(us[name])
            print(json.dumps(dict(model="lenet5", mask_type=name, num_masks=M if name == "mask" else None, num_bayes_layer=k, batch=B, T=T,
                                  us_per_call=round(med, 1), us_min=round(min(us[name]), 1), us_max=round(max(us[name]), 1),
                                  mcd_samples_per_s=round(B * T / med * 1e6), iters=a.iters, device=torch.cuda.get_device_name(0))), flush=True)


def quantised(a, dev):
    W, I = (int(v) for v in a.quant.split(","))
    # (model, its kernels fp16 / quantised, num_bayes_layer, T): the single-exit pair, then the multi-exit pair (T = 3 and 10: the sample
    # counts of the reference's hardware and software flows)
    single = lambda k: (lambda **kw: bx.LeNet5MC(num_bayes_layer=k, dropout_p=0.25, **kw))
    multi = lambda **kw: bx.LeNet5MCEarlyExit(dropout_p=0.25, **kw)
    plans = [(single(k), ("lenet5_kernel", "qlenet5_kernel"), k, (10, 100)) for k in (1, 3)] + [(multi, ("lenet5_me_kernel", "qlenet5_me_kernel"), 2, (3, 10, 100))]
    for make, kernels, k, samples in plans:
        for B in (250, 1024):
            for T in samples:
                x = synthetic_images(B, 1234, channels=1, size=28).to(dev)
                engines = {}
                for name, kw in (("fp16", {}), ("quant", dict(quant_tbit=W, quant_ibit=I))):
                    torch.manual_seed(0)
                    m = synthetic_weights_(make(**kw), 0).to(dev).eval()
                    engines[name] = (m, m.engine(dev, max_batch=B))
                us = {name: [] for name in engines}
                for it in range(a.warmup + a.iters):
                    for name, (_, eng) in engines.items():
                        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                        e0.record()
                        eng.predict(x, T, seed=1)
                        e1.record()
                        e1.synchronize()
                        if it >= a.warmup:
                            us[name].append(e0.elapsed_time(e1) * 1e3)
                for name, (m, _) in engines.items():
                    med = statistics.median(us[name])
                    print(json.dumps(dict(model=m.family, kernel=kernels[name == "quant"], quant=[W, I] if name == "quant" else None,
                                          num_bayes_layer=k, batch=B, T=T, us_per_call=round(med, 1), us_min=round(min(us[name]), 1),
                                          us_max=round(max(us[name]), 1), mcd_samples_per_s=round(B * T / med * 1e6), iters=a.iters,
                                          device=torch.cuda.get_device_name(0))), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--quant", default="", help="W,I: the quantised model (csrc/qlenet5.hip) beside the fp16 model at equal (k, B, T)")
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--cpu-iters", type=int, default=3)
    ap.add_argument("--T", type=int, default=10)
    ap.add_argument("--early-exit", action="store_true", help="T = 100: predict beside predict_early_exit at three thresholds")
    ap.add_argument("--batch", type=int, default=1024, help="the batch of --early-exit")
    ap.add_argument("--masks", type=int, default=0, help="M > 0: the Masksembles model of M masks beside the MC-dropout model")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("lenet_bench needs a GPU: there is no CPU path to time")
    dev = torch.device("cuda:0")
    if a.early_exit:
        return early_exit(a, dev)
    if a.masks:
        return masksembles(a, dev)
    if a.quant:
        return quantised(a, dev)
    for k in (1, 3, "me"):
        for B in (250, 1024):
            torch.manual_seed(0)
            m = bx.LeNet5MCEarlyExit(dropout_p=0.25) if k == "me" else bx.LeNet5MC(num_bayes_layer=k, dropout_p=0.25)
            m = synthetic_weights_(m, 0).to(dev).eval()
            x = synthetic_images(B, 1234, channels=1, size=28).to(dev)
            eng = m.engine(dev, max_batch=B)
            for _ in range(a.warmup):
                eng.predict(x, a.T, seed=1)
            torch.cuda.synchronize()
            us = []
            for _ in range(a.iters):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                eng.predict(x, a.T, seed=1)
                e1.record()
                e1.synchronize()
                us.append(e0.elapsed_time(e1) * 1e3)
            med = statistics.median(us)
            row = dict(model=m.family, num_bayes_layer=2 if k == "me" else k, batch=B, T=a.T, us_per_call=round(med, 1), us_min=round(min(us), 1), us_max=round(max(us), 1),
                       mcd_samples_per_s=round(B * a.T / med * 1e6), iters=a.iters, device=torch.cuda.get_device_name(0))
            if k == 1 and a.cpu_iters:      # the oracle has site C only
                torch.manual_seed(0)
                o = synthetic_weights_(ox.LeNet5MC(dropout_p=0.25), 0)
                xc = x.cpu()
                mcd.mcd_predict(o, xc, a.T, 1)
                ts = []
                for _ in range(a.cpu_iters):
                    t0 = time.perf_counter()
                    mcd.mcd_predict(o, xc, a.T, 1)
                    ts.append(time.perf_counter() - t0)
                row.update(cpu_oracle_us_per_call=round(statistics.median(ts) * 1e6), cpu_oracle_samples_per_s=round(B * a.T / statistics.median(ts)),
                           cpu_threads=torch.get_num_threads(), cpu_cores=os.cpu_count())
            print(json.dumps(row), flush=True)


if __name__ == "__main__":
    main()
