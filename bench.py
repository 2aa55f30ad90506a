#!/usr/bin/env python3
"""Headline benchmark: MCD-samples/s (T x images / s) + ECE, ResNet-18 multi-exit, T = 100.

Workload (BASELINE.json configs[2]): ResNet18MCEarlyExit, CIFAR-10 shape (C=10), dropout="block" +
exit dropout, p=0.25, batch 250 (the reference's test batch, SA/train/hyperparameters.py:265-266),
T=100 Monte-Carlo samples, synthetic N(0,1) images and seeded synthetic weights.

One "step" = one batch through the whole hot path: deterministic prefix once, T masked suffix
passes (folded into the GEMM M dimension in chunks), per-exit softmax moments, finalize to
mean / variance.  Inputs are resident in HBM before the timed region.  With N GPUs the T samples
are sharded across ranks (strong scaling, total work fixed) and the float64 moment buffers are
combined with ONE all-reduce over RCCL per step.  Consecutive steps alternate between two engines / streams (--in-flight 2,
engine.BatchesInFlight): the launch-bound once-per-batch prefix of step k+1 runs beside the suffix of step k; every step still
does all of its own work inside the timed region and its results are bit for bit the one-stream ones.

    python bench.py --gpus 1 --steps 10 --warmup 3
    python bench.py --gpus 1 --steps 10 --warmup 3 --full   # + roofline, CPU baseline, other engines, RCCL probe (see below)
    python bench.py --gpus 1 --steps 10 --warmup 3 --dump-outputs DIR     # + the last timed step's mean / var / logit_mean as DIR/*.npy
    python bench.py --gpus 8 --steps 10 --warmup 3          # starts its 8 rank processes itself (fresh children, torch.distributed.run)
    python -m torch.distributed.run --nnodes=1 --nproc-per-node 8 --master-addr 127.0.0.1 --master-port P \\
        bench.py --gpus 8 --steps 10 --warmup 3             # or under a launcher: RANK / LOCAL_RANK / WORLD_SIZE from the env

Prints ONE JSON line (rank 0).  A plain run sets up, warms up, times the --steps steps and prints the headline: `value`, `ms_per_step`
(wall time of the timed steps / --steps), the per-step completion spread, the engine type and the ECE of the last step.  Everything
that takes runs of its own is measured only with --full: `roofline`, `cpu_baseline`, `parity` / `value_at_tolerance` and
`allreduce_us_1rank`.  `roofline` is the DOMINANT kernel family of the step (the conv family with the largest
share of the step time: conv3x3_pw / conv_igemm_wide / conv3x3_patch / conv_igemm): algorithmic FLOPs (or, where the HBM
roofline is the tighter one, bytes) per launch / its average launch duration, measured by the library with HIP events on the
launch stream in a separate profiled step right after the timed region (event records around every launch would perturb
the timed steps); `all_conv_launches`, `whole_step` and `by_kernel` give the same for all conv launches, the whole timed
step and each family.  `traffic` and the per-kernel MFMA-busy share are quoted from the committed rocprofv3 PMC passes
of this same command (profiles/, tools/profile_all.sh).  `cpu_baseline` is the CPU oracle (a port of the reference loop,
ATen's own RNG) timed on this box's host cores on a bounded sample, at N=1 only.
"""
import argparse
import json
import os
import sys
import time

if os.environ.get("BENCH_RANK_MARK_DIR") and "RANK" in os.environ:      # tests: "rank r of the job was started" (before the slow imports)
    open(os.path.join(os.environ["BENCH_RANK_MARK_DIR"], "rank" + os.environ["RANK"]), "w").close()

import numpy as np
import torch

ROOT = os.path.dirname(os.path.abspath(__file__))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

MFMA_PEAK_TFLOPS = 2500.0       # dense fp16/bf16, MI355X_MICROARCH.md §Chip-level parameters
HBM_PEAK_GBS = 8000.0           # HBM3E, same table
LAUNCH_BOUND_MS = 1.5           # a rank's step under this is launch-bound: three batches in flight + one hipGraph replay per step (round 6: measured on the
                                # exit-only ResNet-18 — probe 1.1 ms, +5.5 % — and VGG-19 — 1.2 ms, +4 % —; neutral at the Masksembles config's 2.2 ms)
MODEL_KW = dict(dropout_exit=True, dropout="block", dropout_p=0.25, out_dim=10)
DUMP_CAP_BYTES = 64 << 20       # --dump-outputs writes at most this much

# name -> (package class, oracle class, kwargs, batch, T, description).  The default is the configuration BASELINE.json's
# metric is quoted on; the others are measurement aids for the remaining GPU configs (not the driver's bench line).
WORKLOADS = {
    "resnet18_me": ("bayesnn_fpga_amd.models.resnet18.resnet18:ResNet18MCEarlyExit", "oracle.resnet18:ResNet18MCEarlyExit",
                    MODEL_KW, 250, 100,
                    "ResNet18MCEarlyExit C=10 dropout=block+exit p=0.25, batch 250 x T=100 (BASELINE configs[2])"),
    "vgg11": ("bayesnn_fpga_amd.models.extra:VGG11MC", "oracle.extra_models:VGG11MC",
              dict(num_bayes_layer=3, dropout_p=0.25, out_dim=10), 250, 30,
              "VGG11MC (build-defined) C=10, 3 dropout sites p=0.25, batch 250 x T=30 (BASELINE configs[1])"),
    "resnet18_masksembles": ("bayesnn_fpga_amd.models.resnet18.resnet18:ResNet18MCEarlyExit",
                             "oracle.resnet18:ResNet18MCEarlyExit",
                             dict(dropout_exit=True, dropout="block", dropout_p=0.25, out_dim=100, mask_type="mask",
                                  num_masks=8, mask_scale=4.0), 250, 8,
                             "ResNet18MCEarlyExit C=100 Masksembles M=8 block+exit, batch 250 x T=8 (BASELINE configs[3])"),
    "resnet18_exit_only": ("bayesnn_fpga_amd.models.resnet18.resnet18:ResNet18MCEarlyExit", "oracle.resnet18:ResNet18MCEarlyExit",
                           dict(dropout_exit=True, dropout=None, dropout_p=0.25, out_dim=100), 250, 10,
                           "ResNet18MCEarlyExit C=100, exit-only dropout p=0.25, batch 250 x T=10 — the configuration every run of the paper uses "
                           "(Software_Artifact/script_figs/journal_script.sh:10-63, SA/train/hyperparameters.py:111-114,265-274)"),
    "resnet18_layer": ("bayesnn_fpga_amd.models.resnet18.resnet18:ResNet18MCEarlyExit", "oracle.resnet18:ResNet18MCEarlyExit",
                       dict(dropout_exit=True, dropout="layer", dropout_p=0.25, out_dim=10), 250, 100,
                       "ResNet18MCEarlyExit C=10 dropout=layer+exit p=0.25 (11 sites, SA/models/resnet18/resnet18.py:281-288), batch 250 x T=100 "
                       "(the headline's T and C, so that the two insertion modes compare directly)"),
    "vgg19_me": ("bayesnn_fpga_amd.models.vgg19.vgg19:VGG19MCEarlyExit", "oracle.vgg19:VGG19MCEarlyExit",
                 dict(dropout_exit=True, dropout=None, dropout_p=0.25, out_dim=100), 250, 100,
                 "VGG19MCEarlyExit C=100, exit dropout p=0.25 (the only mode the reference can construct), batch 250 x T=100"),
    "resnet50_me": ("bayesnn_fpga_amd.models.extra:ResNet50MCEarlyExit", "oracle.extra_models:ResNet50MCEarlyExit",
                    MODEL_KW, 250, 64,
                    "ResNet50MCEarlyExit (build-defined) C=10 dropout=block+exit p=0.25, batch 250 x T=64 "
                    "(one GPU's share of BASELINE configs[4])"),
}


def _load(spec):
    import importlib
    mod, name = spec.split(":")
    return getattr(importlib.import_module(mod), name)


def parse():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--workload", choices=sorted(WORKLOADS), default="resnet18_me")
    ap.add_argument("--batch", type=int, default=0, help="images per batch (0 = the workload's)")
    ap.add_argument("--T", type=int, default=0, help="MC samples per image (0 = the workload's)")
    ap.add_argument("--chunk", type=int, default=0, help="MC samples folded per suffix launch (0 = engine default)")
    ap.add_argument("--seed", type=int, default=42)
    ap.add_argument("--dtype", choices=("auto", "f16", "bf16", "f16x2", "bf16x3"), default="auto",
                    help="auto (default): the PRODUCT's choice — engine_dtype='auto' calibrates fp16 against f16x2 on the bench batch and keeps fp16 only under "
                         "5e-4 (models/_engine_mixin.py); on the synthetic bench weights that is f16, and the line says so (config.engine_dtype).  "
                         "f16 / bf16: 16-bit activations and conv weights (bf16 is reported next to f16); "
                         "f16x2 / bf16x3: the split engines (fp32 activations, 16-bit head + tail operands, three MFMAs per K-step: csrc/conv_split.hip)")
    ap.add_argument("--no-cpu-baseline", action="store_true", help="--full: skip the CPU baseline and the other 16-bit engine")
    ap.add_argument("--no-parity-leg", action="store_true",
                    help="--full, N = 1: skip the tolerance leg (engine_dtype='auto' on the bench model and on its trained-like twin, and the rate of the engine "
                         "auto picks there: `parity_engine` / `value_at_tolerance`)")
    ap.add_argument("--cpu-procs", type=int, default=8, help="processes of the multi-process CPU-baseline sample (slices of the batch, 16 threads each; 0 = skip)")
    ap.add_argument("--cpu-worker", default="", help=argparse.SUPPRESS)      # internal: "lo,hi,T,threads" — one slice of the multi-process CPU baseline
    ap.add_argument("--backend", default="nccl", help="torch.distributed backend (nccl = RCCL; gloo only for the 1-GPU dry run)")
    ap.add_argument("--share-gpu", action="store_true",
                    help="dry run of the N>1 code path on a 1-GPU box: every rank uses cuda:0 (needs --backend gloo)")
    ap.add_argument("--cpu-T", type=int, default=10, help="MC passes of the bounded CPU-baseline sample")
    ap.add_argument("--cpu-1t-images", type=int, default=16, help="images of the 1-thread CPU-baseline sample (0 = skip)")
    ap.add_argument("--in-flight", type=int, default=0,
                    help="batches in flight: consecutive steps alternate between this many engines / streams (engine.BatchesInFlight), so "
                         "the once-per-batch prefix of step k+1 runs beside the suffix of step k; 1 = one stream; 0 (default) = decided by "
                         "measurement: a rank's step is timed once before the warm-up — under 1.5 ms it is launch-bound and gets 3 in flight + "
                         "one hipGraph replay per step (VGG-11, one Masksembles mask per GPU), else 2 eager (the ResNets at T = 100)")
    ap.add_argument("--no-graph", action="store_true", help="never replay a step as a hipGraph (overrides the measured choice)")
    ap.add_argument("--macro", type=int, default=1,
                    help="loader batches carried by one step: the engine batch is macro x the workload's 250 images (SURVEY 8.5: config 4's share "
                         "of eight ranks is 31 images x 8 masks per 250-image batch, 0.6 ms of 25 launches — a macro-batch gives a rank enough work)")
    ap.add_argument("--graph", action="store_true",
                    help="each batch step (zero, prefix, suffix chunks, finalize) is ONE hipGraph replay (engine.BatchesInFlight.predict_graphed): "
                         "takes the launch floor out of the launch-bound small-model configs (VGG-11, one Masksembles mask per GPU); with more "
                         "than one rank the graph holds the rank's share and the all-reduce + finalize follow the replay eagerly")
    ap.add_argument("--partition", choices=("auto", "samples", "images"), default="auto",
                    help="how a batch x T samples is split over the ranks (sharding.partition): auto = by samples while T > ranks, by images otherwise")
    ap.add_argument("--no-rccl-probe", action="store_true", help="--full, N = 1: skip the one-rank RCCL probe (allreduce_us_1rank)")
    ap.add_argument("--rccl-probe-only", action="store_true", help="N = 1: run only the one-rank RCCL probe and print its JSON (tests)")
    ap.add_argument("--dump-mean", default="", help="rank 0 writes the final predictive mean [E,B,C] float64 to this .npy (tests)")
    ap.add_argument("--dump-outputs", default="", metavar="DIR",
                    help="rank 0 writes what the last timed step returned (mean / var / logit_mean, float64 [E,B,C]) as DIR/<name>.npy; "
                         f"over {DUMP_CAP_BYTES >> 20} MB in all, a fixed seeded sample of the images")
    ap.add_argument("--full", action="store_true",
                    help="also measure what the headline does not need, each in runs of its own after the timed steps: the per-kernel "
                         "roofline (a profiled step), at N = 1 the CPU baseline and the other 16-bit engine (--no-cpu-baseline), the tolerance "
                         "leg (--no-parity-leg) and the one-rank RCCL probe (--no-rccl-probe)")
    a = ap.parse_args()
    if a.steps < 1:
        ap.error("--steps >= 1")
    return a


def dump_outputs(path, outs, seed=0):
    """--dump-outputs: the arrays the timed path returned in its last step, one DIR/<name>.npy each.  Over DUMP_CAP_BYTES in all,
    the same fixed, seeded sample of the images (axis 1 of [E, B, C]) is written for every array."""
    os.makedirs(path, exist_ok=True)
    total = sum(v.nbytes for v in outs.values())
    keep = None
    if total > DUMP_CAP_BYTES:
        B = next(iter(outs.values())).shape[1]
        keep = np.sort(np.random.default_rng(seed).choice(B, max(1, B * DUMP_CAP_BYTES // total), replace=False))
    for name, v in outs.items():
        np.save(os.path.join(path, f"{name}.npy"), v if keep is None else v[:, keep])


def _family_match(kernel_name, family):
    """rocprof kernel names ('conv_igemm_wide_persist_kernel<16, false>') -> the library's kernel families."""
    stem = family[:-len("_kernel")] if family.endswith("_kernel") else family
    if not kernel_name.startswith(stem):
        return False
    return stem != "conv_igemm" or kernel_name.startswith("conv_igemm_kernel")      # conv_igemm is a prefix of conv_igemm_wide


def hbm_traffic(workload, launches_per_step, family=None):
    """HBM bytes per launch of the conv kernels (or of one family) from the committed rocprofv3 PMC passes of this same
    command (tools/pmc_summary.py -> profiles/hbm_traffic_<workload>.json; FETCH_SIZE x2 + WRITE_SIZE, KiB -> bytes).
    None when absent or collected for another launch count."""
    path = os.path.join(ROOT, "profiles", f"hbm_traffic_{workload}.json")
    if not os.path.exists(path):
        return None, None
    allk = {k: v for k, v in json.load(open(path))["kernels"].items() if k.startswith(("conv_igemm", "conv3x3_patch", "conv3x3_pw", "conv3x3_s2", "conv1x1_stream", "conv1x1_seam", "conv_split"))}
    n_all = sum(v["launches"] for v in allk.values())
    if n_all == 0 or n_all % launches_per_step:
        return None, None                   # collected for another batch / T / chunking: do not quote it
    ks = allk if family is None else {k: v for k, v in allk.items() if _family_match(k, family)}
    n = sum(v["launches"] for v in ks.values())
    if n == 0:
        return None, None
    return sum(v["hbm_bytes_per_launch"] * v["launches"] for v in ks.values()) / n, os.path.relpath(path, ROOT)


def pmc_sq(workload, family):
    """Launch-weighted SQ/GRBM figures of one conv kernel family from the same committed PMC summary (third pass of
    tools/profile_bench.sh): MFMA-pipe busy share and effective shader clock.  {} when absent."""
    path = os.path.join(ROOT, "profiles", f"hbm_traffic_{workload}.json")
    if not os.path.exists(path):
        return {}
    ks = [v for k, v in json.load(open(path))["kernels"].items() if _family_match(k, family) and "sq" in v    # (wide covers ..._persist)
          and v["sq"]["mfma_busy_share"] > 0.05]
    n = sum(v["launches"] for v in ks)
    if not n:
        return {}
    return {"mfma_busy_share_pmc": round(sum(v["sq"]["mfma_busy_share"] * v["launches"] for v in ks) / n, 4),
            "effective_clock_ghz_pmc": round(sum(v["sq"]["effective_clock_ghz"] * v["launches"] for v in ks) / n, 3)}


def rocprof_family(workload, family, launches_per_step):
    """The committed `rocprofv3 --kernel-trace --stats` summary of this same command (the newest profiles/rNN_<workload>_kernel_stats.csv):
    the launches of one conv family — (name of its kernel with the most device time as rocprof prints it, without template arguments;
    average launch duration in ms over ALL the family's kernels; calls; file).  None when absent or collected for another launch count."""
    import csv
    import glob
    import re
    files = sorted(glob.glob(os.path.join(ROOT, "profiles", f"r[0-9][0-9]_{workload}_kernel_stats.csv")))
    if not files:
        return None
    tot, calls, by_name = 0.0, 0, {}
    for row in csv.DictReader(open(files[-1])):
        name = re.sub(r"^void ", "", row["Name"]).split("<")[0].split("(")[0]
        if _family_match(name, family):
            tot += float(row["TotalDurationNs"])
            calls += int(row["Calls"])
            by_name[name] = by_name.get(name, 0.0) + float(row["TotalDurationNs"])
    if not calls or calls % max(launches_per_step, 1):
        return None
    return max(by_name, key=by_name.get), tot / calls * 1e-6, calls, os.path.relpath(files[-1], ROOT)


def rocprof_top_symbol(workload):
    """The single kernel SYMBOL (template arguments included) with the most device time in the committed rocprofv3 summary of this command —
    the family view of `roofline` can hide it (round-5 review: by family the headline's dominant kernel is conv3x3_pwp, by symbol the 16x16
    instantiation of conv3x3_patch).  {name, calls, avg_ms, share_of_kernel_time} or None."""
    import csv
    import glob
    import re
    files = sorted(glob.glob(os.path.join(ROOT, "profiles", f"r[0-9][0-9]_{workload}_kernel_stats.csv")))
    if not files:
        return None
    rows = [(re.sub(r"^void ", "", r["Name"]).split("(")[0], int(r["Calls"]), float(r["TotalDurationNs"])) for r in csv.DictReader(open(files[-1]))]
    total = sum(r[2] for r in rows) or 1.0
    conv = [r for r in rows if r[0].startswith("conv")]
    if not conv:
        return None
    nm, calls, ns = max(conv, key=lambda r: r[2])
    return {"name": nm, "calls": calls, "avg_ms": round(ns / calls * 1e-6, 4), "share_of_kernel_time": round(ns / total, 4), "source": os.path.relpath(files[-1], ROOT)}


def physical_cores():
    """Physical cores of this host (unique (package, core) pairs of /proc/cpuinfo); None when it cannot be told."""
    try:
        ids, phys = set(), None
        for ln in open("/proc/cpuinfo"):
            if ln.startswith("physical id"):
                phys = ln.split(":")[1].strip()
            elif ln.startswith("core id"):
                ids.add((phys, ln.split(":")[1].strip()))
        return len(ids) or None
    except OSError:
        return None


def cpu_baseline_1thread(wl, images, T, seed):
    """The same oracle loop on ONE thread (SURVEY §8.4 asks for the 1-thread figure next to the all-cores one), on a
    smaller bounded sample (``images`` images x T passes)."""
    from bayesnn_fpga_amd.synthetic import synthetic_images, synthetic_weights_
    from oracle import mcd
    n = torch.get_num_threads()
    torch.set_num_threads(1)
    try:
        torch.manual_seed(0)
        np.random.seed(0)
        m = synthetic_weights_(_load(wl[1])(**wl[2]), 0)
        x = synthetic_images(images, seed=1234)
        from oracle.layers import MCDropout
        MCDropout.native_rng = True
        mcd.mcd_predict(m, x[:2], 1, seed)
        t0 = time.perf_counter()
        mcd.mcd_predict(m, x, T, seed)
        return images * T / (time.perf_counter() - t0)
    finally:
        MCDropout.native_rng = False
        torch.set_num_threads(n)


def best_thread_count(m, x, seed, candidates):
    """ATen's CPU convolutions do not scale to every core of a 2-socket host at batch 250 (measured: 128 threads are
    SLOWER than one).  The baseline should be the reference's loop at its best, so a short sweep (2 passes each) picks the
    intra-op thread count; the all-cores figure is reported next to it."""
    import copy
    from oracle import mcd
    from oracle.layers import MCDropout
    n0 = torch.get_num_threads()
    rates = {}
    MCDropout.native_rng = True
    try:
        for n in candidates:
            torch.set_num_threads(n)
            mm = copy.deepcopy(m)
            mcd.mcd_predict(mm, x[:8], 1, seed)
            t0 = time.perf_counter()
            mcd.mcd_predict(mm, x, 2, seed)
            rates[n] = x.shape[0] * 2 / (time.perf_counter() - t0)
    finally:
        MCDropout.native_rng = False
        torch.set_num_threads(n0)
    return max(rates, key=rates.get), rates


def cpu_baseline(wl, batch, T, seed):
    """The oracle (port of FullAnalysis._get_output, T sequential full forwards per batch, fp32) on
    the host cores.  Returns (MCD-samples/s, threads, mean probs, {threads: rate} of the sweep)."""
    from bayesnn_fpga_amd.synthetic import synthetic_images, synthetic_weights_
    from oracle import mcd
    torch.manual_seed(0)
    np.random.seed(0)
    m = synthetic_weights_(_load(wl[1])(**wl[2]), 0)
    x = synthetic_images(batch, seed=1234)
    import copy
    mcd.mcd_predict(copy.deepcopy(m), x[:8], 1, seed)   # warm the allocator / oneDNN primitives (on a copy: Masksembles
                                                        # layers count their calls, the timed model must start at mask 0)
    r = mcd.mcd_predict(m, x, T, seed)                   # parity leg: Philox masks, the same as the GPU's (not timed)
    # timing leg: the reference's own loop — T sequential full forwards with ATen's F.dropout as the RNG
    # (results_analyzer.py:236-248); the numpy Philox restatement above costs more than the convolutions themselves
    from oracle.layers import MCDropout
    n_all = torch.get_num_threads()
    cand = sorted({n for n in (n_all, n_all // 2, n_all // 4, n_all // 8, 16, 8) if 1 <= n <= n_all}, reverse=True)
    best, sweep = best_thread_count(m, x, seed, cand)
    MCDropout.native_rng = True
    torch.set_num_threads(best)
    try:
        t0 = time.perf_counter()
        mcd.mcd_predict(copy.deepcopy(m), x, T, seed)
        dt = time.perf_counter() - t0
    finally:
        MCDropout.native_rng = False
        torch.set_num_threads(n_all)
    return batch * T / dt, best, r["mean"], sweep


def cpu_worker(a):
    """One slice of the multi-process CPU baseline (started by ``cpu_baseline_multiproc``; touches no GPU API): builds the oracle model, warms up,
    prints "ready", waits for "go" on stdin, runs the reference's loop on images [lo, hi) and prints the seconds it took."""
    lo, hi, T, threads = (int(v) for v in a.cpu_worker.split(","))
    torch.set_num_threads(threads)
    from bayesnn_fpga_amd.synthetic import synthetic_images, synthetic_weights_
    from oracle import mcd
    from oracle.layers import MCDropout
    wl = WORKLOADS[a.workload]
    torch.manual_seed(0)
    np.random.seed(0)
    m = synthetic_weights_(_load(wl[1])(**wl[2]), 0)
    x = synthetic_images(a.batch or wl[3], seed=1234)[lo:hi]
    MCDropout.native_rng = True
    mcd.mcd_predict(m, x[:2], 1, a.seed)
    print("ready", flush=True)
    sys.stdin.readline()
    t0 = time.perf_counter()
    mcd.mcd_predict(m, x, T, a.seed)
    print(f"done {time.perf_counter() - t0:.6f}", flush=True)


def cpu_baseline_multiproc(a, batch, T, procs, threads=16):
    """The same oracle loop as N processes x ``threads`` intra-op threads over contiguous slices of the batch (round-5 review, weak #8: ATen's
    CPU convolutions at batch 250 barely scale inside ONE process on this 2-socket host — 1 thread 148, 32 threads 362, 128 threads 78
    MCD-samples/s — so a single process under-states what the host can do).  All children are warm before the clock starts; the rate is
    batch x T / wall time until the LAST slice is done.  Returns (MCD-samples/s, processes, threads) or (None, ...) on any failure."""
    import subprocess
    from bayesnn_fpga_amd.sharding import shard_range
    procs = max(1, min(procs, batch))
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE")}
    env["OMP_NUM_THREADS"] = str(threads)
    kids = []
    try:
        for r in range(procs):
            lo, hi = shard_range(batch, r, procs)
            cmd = [sys.executable, os.path.abspath(__file__), "--workload", a.workload, "--seed", str(a.seed), "--batch", str(batch),
                   "--cpu-worker", f"{lo},{hi},{T},{threads}"]
            kids.append(subprocess.Popen(cmd, stdin=subprocess.PIPE, stdout=subprocess.PIPE, stderr=subprocess.DEVNULL, text=True, env=env))
        for k in kids:
            if k.stdout.readline().strip() != "ready":
                raise RuntimeError("a CPU-baseline worker did not come up")
        t0 = time.perf_counter()
        for k in kids:
            k.stdin.write("go\n")
            k.stdin.flush()
        for k in kids:
            if not k.stdout.readline().startswith("done"):
                raise RuntimeError("a CPU-baseline worker failed")
        dt = time.perf_counter() - t0
        return batch * T / dt, procs, threads
    except Exception:                  # noqa: BLE001 — a reported baseline, never a reason to lose the bench line
        return None, procs, threads
    finally:
        for k in kids:
            try:
                k.stdin.close()
                k.wait(timeout=30)
            except Exception:          # noqa: BLE001
                k.kill()


HEAD_NAMES = ("ex1linear", "ex2linear", "ex3linear", "linear")


def tolerance_leg(model, dev, x, B, T, seed, steps, gain=24.0, rec=None):
    """The rate AT north_star's tolerance (round-5 review, weak #1 / next #1d): what engine_dtype="auto" — the product default — decides on
    the bench model and on its TRAINED-LIKE twin (every classifier x 24: max prob >= 0.99 on most images, where fp16 measures 5e-3 against
    the oracle, tests/test_auto_engine.py), and the whole-step rate of the engine it picks for the twin, timed like the headline (two
    batches in flight, HIP-resident inputs).  Read: `value` holds on weights where fp16 is good enough — auto proves that on the first
    batch —, `value_at_tolerance` on trained-like ones."""
    import copy
    import warnings
    from bayesnn_fpga_amd.engine import BatchesInFlight
    out = {}
    if rec is None:
        rec = model.calibrate_engine_dtype(dev, x, samples=min(T, 32))
    out["auto_on_bench_model"] = {k: rec[k] for k in ("dtype", "dmean", "dvar", "tol", "images", "samples")}
    if not all(hasattr(model, n) for n in HEAD_NAMES):
        return out
    twin = copy.deepcopy(model)
    with torch.no_grad():
        for n in HEAD_NAMES:
            getattr(twin, n).weight.mul_(gain)
    twin.invalidate_engine()
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        rec2 = twin.calibrate_engine_dtype(dev, x, samples=min(T, 32))
    out["auto_on_trained_like_twin"] = {k: rec2[k] for k in ("dtype", "dmean", "dvar", "tol", "images", "samples")}
    out["parity_engine"] = rec2["dtype"]
    pipe = BatchesInFlight(twin, dev, n=2, max_batch=B, dtype=rec2["dtype"])
    try:
        for _ in range(2):
            pipe.step(x, T, seed)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(steps):
            pipe.step(x, T, seed)
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        for e in pipe.engines:
            e.check_finite()
    finally:
        pipe.close()
    out["value_at_tolerance"] = round(B * T * steps / dt, 1)
    out["ms_per_step_at_tolerance"] = round(dt / steps * 1e3, 3)
    out["steps_at_tolerance"] = steps
    out["note"] = (f"engine_dtype='auto' keeps {rec['dtype']!r} on the bench model (fp16 vs f16x2 on the first batch: {rec['dmean']:.1e} <= {rec['tol']:.0e}) and picks "
                   f"{rec2['dtype']!r} on the twin with classifiers x {gain:g} ({rec2['dmean']:.1e}); value_at_tolerance = whole-step rate of that engine")
    return out


def rccl_probe_one_rank(pipe, x, T, seed, reps=50):
    """RCCL on ONE GPU, on exactly the streams and buffers the N-GPU path uses (the only part of that path a 1-GPU box can execute):
    a process group of one rank over backend "nccl" (= RCCL), then
      * the float64 all-reduce of the [3, E, B, C] moment buffer issued from EACH of the in-flight side streams, timed with HIP events on
        that stream (`allreduce_us`), and a whole eager step with the collective in it (sharding.accumulate_partitioned,
        always_reduce) compared bit for bit with the same step without it (a sum over one rank);
      * the same behind a hipGraph replay of the step (BatchesInFlight.predict_graphed: replay, all-reduce, finalize on the slot's stream).
    Returns a dict (or {"error": ...}: the probe never fails the bench).  Leaves the process group destroyed."""
    import socket
    import torch.distributed as dist
    from bayesnn_fpga_amd.sharding import accumulate_partitioned
    if dist.is_initialized():
        return {"error": "a process group is already initialised"}
    dev = pipe.device
    out = {}
    try:
        with socket.socket() as s:
            s.bind(("127.0.0.1", 0))
            port = s.getsockname()[1]
        os.environ["MASTER_ADDR"], os.environ["MASTER_PORT"] = "127.0.0.1", str(port)
        os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
        t0 = time.perf_counter()
        dist.init_process_group("nccl", rank=0, world_size=1, device_id=dev)
        first = torch.zeros(1, dtype=torch.float64, device=dev)
        dist.all_reduce(first)                      # the communicator is created by its first collective (default stream)
        torch.cuda.synchronize(dev)
        out["init_plus_first_collective_ms"] = round((time.perf_counter() - t0) * 1e3, 1)
        B = x.shape[0]
        per_stream, identical = [], True
        for i, (e, st) in enumerate(zip(pipe.engines, pipe.streams)):
            st = st if st is not None else torch.cuda.current_stream(dev)
            S, S_ref = e.new_moments(B), e.new_moments(B)
            st.wait_stream(torch.cuda.current_stream(dev))
            with torch.cuda.stream(st):
                e.accumulate(x, S_ref, 0, T, seed)
                accumulate_partitioned(e, x, S, T, seed, always_reduce=True)        # the step with the collective behind it
                ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
                for _ in range(5):
                    dist.all_reduce(S_ref)
                ev[0].record(st)
                for _ in range(reps):
                    dist.all_reduce(S_ref)
                ev[1].record(st)
            st.synchronize()
            per_stream.append(round(ev[0].elapsed_time(ev[1]) / reps * 1e3, 2))
            identical = identical and bool(torch.equal(S, S_ref))
        out["allreduce_us"] = per_stream
        out["buffer_bytes"] = int(S.numel() * 8)
        out["eager_step_with_allreduce_equals_step_without"] = identical
        # behind a graph replay (two submissions per slot: capture, then a replay)
        plain = pipe.engines[0].predict(x, T, seed)
        torch.cuda.synchronize(dev)
        same, graph_us = True, []
        for _ in range(2 * len(pipe.engines)):
            r = pipe.predict_graphed(x, T, seed, group=dist.group.WORLD, always_reduce=True)
            pipe.last_stream.synchronize()
            same = same and all(bool(torch.equal(r[k], plain[k])) for k in ("mean", "var", "logit_mean"))
        st = pipe.last_stream
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
        with torch.cuda.stream(st):
            Sg = pipe.engines[0].new_moments(B)
            ev[0].record(st)
            for _ in range(reps):
                dist.all_reduce(Sg)
            ev[1].record(st)
        st.synchronize()
        graph_us = round(ev[0].elapsed_time(ev[1]) / reps * 1e3, 2)
        out["graph_replay_plus_allreduce_equals_eager"] = same
        out["allreduce_us_on_the_graph_stream"] = graph_us
        out["backend"] = "nccl (RCCL), world_size 1"
    except Exception as exc:           # noqa: BLE001 — measurement aid: report, never fail the bench line
        out["error"] = f"{type(exc).__name__}: {exc}"[:300]
    finally:
        try:
            if dist.is_initialized():
                dist.destroy_process_group()
        except Exception:              # noqa: BLE001
            pass
    return out


def rccl_probe_in_a_child(a, timeout=240):
    """The one-rank RCCL probe in a CHILD process (`bench.py --rccl-probe-only`, an ordinary subprocess: this process keeps running and
    never re-execs itself): a communicator that hangs or dies at start-up or tear-down costs the bench line `timeout` seconds and an
    {"error": ...} entry, never the line itself."""
    import subprocess
    cmd = [sys.executable, os.path.abspath(__file__), "--gpus", "1", "--rccl-probe-only", "--workload", a.workload, "--in-flight", str(a.in_flight),
           "--dtype", a.dtype, "--seed", str(a.seed), "--macro", str(a.macro)]
    for flag, val in (("--batch", a.batch), ("--T", a.T), ("--chunk", a.chunk)):
        if val:
            cmd += [flag, str(val)]
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT")}
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    try:
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=timeout, env=env)
        lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
        if r.returncode != 0 or not lines:
            return {"error": f"probe child exited with {r.returncode}: {r.stderr[-200:]}"}
        return json.loads(lines[-1])
    except subprocess.TimeoutExpired:
        return {"error": f"probe child did not finish within {timeout} s"}
    except Exception as exc:           # noqa: BLE001
        return {"error": f"{type(exc).__name__}: {exc}"[:300]}


def launch_ranks(n):
    """`python bench.py --gpus N` from a plain shell: start the N rank processes ourselves — fresh children through
    torch.distributed.run, one per GPU, rendezvous on 127.0.0.1 — relay their output (rank 0 prints the JSON line) and exit
    with their code.  Nothing in THIS process has touched the GPU (no torch.cuda call, no HIP call), and it never re-execs
    itself: the children are ordinary subprocesses."""
    import subprocess
    env = dict(os.environ)
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")      # dmabuf IPC (RCCL between processes needs it on this host driver)
    env.setdefault("OMP_NUM_THREADS", "1")
    # --standalone: torchrun's own c10d rendezvous on a port IT binds (a port probed here and released could be taken before the agent
    # binds it: one flaky 2-rank test in six rounds); --local-addr 127.0.0.1: the container hostname may not resolve
    cmd = [sys.executable, "-m", "torch.distributed.run", "--standalone", "--local-addr", "127.0.0.1", "--nnodes=1", "--nproc-per-node", str(n),
           os.path.abspath(__file__), *sys.argv[1:]]
    return subprocess.run(cmd, env=env).returncode


def main():
    a = parse()
    if a.cpu_worker:
        return cpu_worker(a)
    if a.gpus < 1:
        raise SystemExit("--gpus >= 1")
    if a.gpus > 1 and "WORLD_SIZE" not in os.environ:
        sys.exit(launch_ranks(a.gpus))
    rank = int(os.environ.get("RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    local = int(os.environ.get("LOCAL_RANK", "0"))
    if world != a.gpus:
        raise SystemExit(f"--gpus {a.gpus} but WORLD_SIZE={world}: the launcher's --nproc-per-node and --gpus must agree")
    if a.share_gpu and a.backend == "nccl":
        raise SystemExit("--share-gpu is the 1-GPU dry run of the N>1 path and needs --backend gloo")
    if not torch.cuda.is_available():
        raise SystemExit("bench.py needs an MI355X: the HIP path has no CPU fallback")
    if a.share_gpu:
        local = 0
    torch.cuda.set_device(local)
    dev = torch.device("cuda", local)
    dist = None
    if world > 1:
        import torch.distributed as dist
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        if a.backend == "nccl":
            dist.init_process_group("nccl", rank=rank, world_size=world, device_id=dev)
        else:
            dist.init_process_group(a.backend, rank=rank, world_size=world)
        # the communicator is created by its first collective: do that here, on the default stream, before any step issues an
        # all-reduce from one of the in-flight side streams
        _probe = torch.zeros(1, dtype=torch.float64, device=dev)
        dist.all_reduce(_probe)
        torch.cuda.synchronize()

    from bayesnn_fpga_amd.sharding import accumulate_partitioned, partition, share_kind
    from bayesnn_fpga_amd.synthetic import synthetic_images, synthetic_labels, synthetic_weights_
    from bayesnn_fpga_amd.train.metrics import ece_hist_binary

    wl = WORKLOADS[a.workload]
    kw = wl[2]
    torch.manual_seed(0)
    np.random.seed(0)
    model = synthetic_weights_(_load(wl[0])(**kw), 0).to(dev).eval()
    B, T = (a.batch or wl[3]) * max(a.macro, 1), a.T or wl[4]
    from bayesnn_fpga_amd.engine import BatchesInFlight
    from bayesnn_fpga_amd.sharding import accumulate_share
    if a.in_flight < 0:
        raise SystemExit("--in-flight >= 0")
    x = synthetic_images(B, seed=1234).to(dev)
    auto_rec = None
    if a.dtype == "auto":            # the product default: decided on this batch, outside the timed region, the same on every rank (deterministic)
        import warnings
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            auto_rec = model.calibrate_engine_dtype(dev, x, samples=min(T, 32))      # at the caller's T like FullAnalysis / evaluate (capped at 32)
        a.dtype = auto_rec["dtype"]
        if world > 1:                # one engine type per job: any rank on the split engine moves all of them (same inputs and seeds: a formality)
            a.dtype = model.agree_engine_dtype(dev, a.dtype)
    pipe = BatchesInFlight(model, dev, n=1, max_batch=B, chunk_samples=a.chunk or None, dtype=a.dtype)
    eng = pipe.engines[0]
    pkind = None if a.partition == "auto" else a.partition
    # batches in flight / hipGraph replay: by measurement of THIS rank's share of a step (before the warm-up, outside the timed region);
    # every rank takes the slowest rank's figure, so the group decides together
    S_probe = eng.new_moments(B)
    partition_probe = None
    if dist is not None and pkind is None:
        # --partition auto with several ranks: both splits a rank can take are timed (this rank's share, no collective) and the group
        # takes the one whose SLOWEST rank is faster — on one MI355X rank 0's share of eight at T = 100 measures 2.98 ms by samples and
        # 2.78 ms by images (profiles/r05_share_config4.txt); which wins depends on T, B and the rank count, so it is measured, not assumed
        from bayesnn_fpga_amd.sharding import shard_range
        cands = [k for k in ("samples", "images")
                 if (k == "samples" and T >= world) or (k == "images" and B >= world and all(eng.image_offset_ok(shard_range(B, r, world)[0]) for r in range(world)))]
        if len(cands) == 2:
            ms = [pipe.measure_ms(lambda e, k=k: accumulate_share(e, x, S_probe.zero_(), T, a.seed, 0, rank, world, k)) for k in cands]
            tp = torch.tensor(ms, dtype=torch.float64, device=dev)
            dist.all_reduce(tp, op=dist.ReduceOp.MAX)
            partition_probe = {k: round(float(v), 4) for k, v in zip(cands, tp.tolist())}
            pkind = min(partition_probe, key=partition_probe.get)
        elif cands:
            pkind = cands[0]
    probe_ms = pipe.measure_ms(lambda e: accumulate_share(e, x, S_probe, T, a.seed, 0, rank, world, pkind))
    if dist is not None:
        tprobe = torch.tensor([probe_ms], dtype=torch.float64, device=dev)
        dist.all_reduce(tprobe, op=dist.ReduceOp.MAX)
        probe_ms = float(tprobe.item())
    launch_bound = probe_ms < LAUNCH_BOUND_MS
    a.in_flight = a.in_flight or (3 if launch_bound else 2)
    a.graph = bool(a.graph or (launch_bound and not a.no_graph))
    pipe.grow(a.in_flight)
    del S_probe
    # ("samples", lo, hi) while T > world, else ("images", lo, hi): nobody idles (share_kind: by samples after all when an image share
    # could not start on a whole Philox call of every site)
    share = partition(T, B, rank, world, share_kind(eng, T, B, world, pkind))
    t_lo, t_hi = (share[1], share[2]) if share[0] == "samples" else (0, T)
    Ss = [e.new_moments(B) for e in pipe.engines]

    if a.rccl_probe_only:
        if world != 1:
            raise SystemExit("--rccl-probe-only is the one-rank probe")
        print(json.dumps(rccl_probe_one_rank(pipe, x, T, a.seed)), flush=True)
        return

    def one_batch(e, S):
        S.zero_()
        # the library's N>1 path (bayesnn_fpga_amd/sharding.py): this rank's share into S, then ONE all-reduce (RCCL
        # over xGMI) of the [3,E,B,C] float64 buffer; a single rank skips the collective
        accumulate_partitioned(e, x, S, T, a.seed, kind=pkind)
        return e.finalize(S, T)

    def step():
        # one step = one batch through the whole path; consecutive steps alternate between the engines / streams of `pipe`
        if a.graph:
            return pipe.predict_graphed(x, T, a.seed, kind=pkind, shard=True)
        i = pipe.slot()
        return pipe.submit(lambda e: one_batch(e, Ss[i]))

    def fence():
        if dist is not None:
            dist.barrier()
        torch.cuda.synchronize()

    for _ in range(a.warmup):
        step()
    fence()
    # per-step completion events (the median of >= 10 timed iterations next to the mean): one record per step on the
    # stream the step ran on — no synchronisation inside the timed region, `value` stays K steps / wall
    ev0 = torch.cuda.Event(enable_timing=True)
    evs = [torch.cuda.Event(enable_timing=True) for _ in range(a.steps)]
    ev0.record(torch.cuda.current_stream(dev))
    t0 = time.perf_counter()
    for k in range(a.steps):
        out = step()
        evs[k].record(pipe.last_stream if pipe.last_stream is not None else torch.cuda.current_stream(dev))
    fence()
    dt = time.perf_counter() - t0
    done_ms = [0.0] * a.in_flight + [ev0.elapsed_time(e) for e in evs]     # completion time of step k since the start of the timed region
    # steady-state time per step: with w batches in flight the steps complete in bunches of w (they share the GPU), so the interval is taken
    # over a window of w completions: (done[k] - done[k - w]) / w
    w = a.in_flight
    step_ms = sorted((done_ms[k + w] - done_ms[k]) / w for k in range(len(evs)))
    median_ms = (step_ms[len(step_ms) // 2] + step_ms[(len(step_ms) - 1) // 2]) / 2 if step_ms else 0.0
    if dist is not None:
        tmax = torch.tensor([dt], dtype=torch.float64, device=dev)
        dist.all_reduce(tmax, op=dist.ReduceOp.MAX)
        dt = float(tmax.item())
    outs = {k: v.cpu().numpy() for k, v in out.items()} if rank == 0 else None      # what the last timed step returned

    if a.full:
        # ---- per-kernel profile (rank 0's share of the samples), outside the timed region ----------
        eng.profile(True)
        one_batch(eng, Ss[0])
        torch.cuda.synchronize()
        prof = eng.profile_read()
        eng.profile(False)

    if rank == 0:
        samples = B * T * a.steps
        value = samples / dt
        mean = outs["mean"]
        for e in pipe.engines:
            e.check_finite()                           # non-finite moment sums in any timed step are an error, not a number
        if a.dump_mean:
            np.save(a.dump_mean, mean)
        if a.dump_outputs:
            dump_outputs(a.dump_outputs, outs)
        labels = synthetic_labels(B, kw["out_dim"], seed=1235).numpy()
        onehot = np.eye(kw["out_dim"])[labels]
        line = {
            "metric": "MCD-samples/sec (T x images/s) + ECE, ResNet-18 multi-exit T=100" if a.workload == "resnet18_me"
                      else f"MCD-samples/sec (T x images/s) + ECE, {a.workload} T={T}",
            "value": round(value, 1), "unit": "MCD-samples/s", "n_gpus": world, "steps": a.steps, "warmup": a.warmup,
            "ms_per_step": round(dt / a.steps * 1e3, 3),
            # time per step from the step completions (HIP events on the steps' own streams; windows of `batches_in_flight` completions), rank 0:
            # median / min / max, and the rate the median implies (the first steps of a short run sit on the clock ramp: SURVEY §8.4 asks for
            # the median of >= 10 timed iterations)
            "ms_per_step_median": round(median_ms, 3), "ms_per_step_min": round(step_ms[0], 3) if step_ms else None,
            "ms_per_step_max": round(step_ms[-1], 3) if step_ms else None,
            "value_at_median": round(B * T / (median_ms * 1e-3), 1) if median_ms > 0 else None,
            "higher_is_better": True, "scaling": "strong",
            "vs_baseline": None, "dtype": a.dtype, "data": "synthetic",
            "config": {"workload": wl[5],
                       "engine_dtype": (f"auto -> {a.dtype} (fp16 vs f16x2 on the bench batch: mean {auto_rec['dmean']:.1e} / variance {auto_rec['dvar']:.1e}, kept under "
                                        f"{auto_rec['tol']:.0e})" if auto_rec else a.dtype),
                       "batch": B, "T": T, "chunk_samples": eng.chunk_samples,
                       "workspace_gb": round(eng.workspace_bytes / 2**30, 2), "batches_in_flight": a.in_flight, "hipgraph": bool(a.graph),
                       "macro_batches": a.macro, "rank_step_probe_ms": round(probe_ms, 4), "partition_probe_ms": partition_probe,
                       "pipe": f"3 in flight + one hipGraph replay per step (launch-bound: the probed step is under {LAUNCH_BOUND_MS} ms)" if launch_bound
                               else f"2 eager batches in flight (the probed step is over {LAUNCH_BOUND_MS} ms)",
                       "sharding": (f"T over {world} rank(s)" if share[0] == "samples" else f"images over {world} ranks (T <= ranks)") +
                                   ", one float64 all-reduce per batch"},
            "ece_hist_final_exit": round(ece_hist_binary(mean[-1], onehot), 6),
            "ece_note": "synthetic weights on uniform synthetic labels: plumbing (equal to the CPU oracle's at equal T), not calibration",
            "tflops_executed": round(eng.flops_per_batch(B, T) * a.steps / dt / 1e12, 2),
            "tflops_naive_equiv": round(2.0 * (eng.prefix_macs + eng.suffix_macs) * samples / dt / 1e12, 2),
        }
        if a.full:
            my_T = t_hi - t_lo
            # conv FLOPs of rank 0's profiled step: prefix convs once + suffix convs x its samples
            my_B = B if share[0] == "samples" else share[2] - share[1]      # images of rank 0's profiled step
            conv_flops = 2.0 * my_B * ((eng.prefix_macs) + my_T * (eng.suffix_macs - eng.head_macs - eng.dense_macs))
            conv_ms, conv_launches = prof.get("conv_igemm", (0.0, 0))
            conv_flops -= 2.0 * my_B * eng.stem_macs     # the 3-channel stem runs in its own direct kernel
            achieved = conv_flops / (conv_ms * 1e-3) / 1e12 if conv_ms > 0 else 0.0
            alg_launches = int(conv_launches)            # launches actually made (paired convs are one launch)
            alg_bytes = sum(v["bytes"] for v in eng.conv_families.values())       # what the launches were priced at (lazy-site operands: B images + bits)
            traffic, traffic_src = (hbm_traffic(a.workload, max(alg_launches, 1))
                                    if (world == 1 and not a.batch and not a.T and not a.chunk) else (None, None))
            line["roofline"] = None
            # ---- roofline: the DOMINANT kernel family of the step (largest share of the step time), priced against the roofline
            # that bounds it: algorithmic FLOPs (or bytes) per launch / its average launch duration, HIP events on the launch
            # stream.  `all_conv_launches` is the same for every conv launch together, `by_kernel` per family.
            fam = eng.conv_families
            # the split engines' kernel issues THREE MFMA instructions per algorithmic product (w_lo.x_hi + w_hi.x_lo + w_hi.x_hi): its MFMA
            # roofline in algorithmic FLOPs is a third of the dense peak (`achieved` stays algorithmic, `mfma_work_factor` says so)
            wf = lambda k: 3.0 if k == "conv_split_kernel" else 1.0
            by_kernel = {k: {"launches": int(v["launches"]), "avg_launch_ms": round(v["ms"] / v["launches"], 4),
                             "achieved": round(v["flops"] / (v["ms"] * 1e-3) / 1e12, 1),
                             "mfma_work_factor": wf(k), "peak_algorithmic_tflops": round(MFMA_PEAK_TFLOPS / wf(k), 1),
                             "frac": round(wf(k) * v["flops"] / (v["ms"] * 1e-3) / 1e12 / MFMA_PEAK_TFLOPS, 4),
                             "hbm_gbs_algorithmic": round(v["bytes"] / (v["ms"] * 1e-3) / 1e9, 1),
                             "hbm_frac": round(v["bytes"] / (v["ms"] * 1e-3) / 1e9 / HBM_PEAK_GBS, 4),
                             "flop_per_byte": round(v["flops"] / max(v["bytes"], 1.0), 1),
                             "algorithmic_flops_per_launch": round(v["flops"] / v["launches"]),
                             "algorithmic_bytes_per_launch": round(v["bytes"] / v["launches"]),
                             "bound": "mfma" if wf(k) * v["flops"] / MFMA_PEAK_TFLOPS / 1e12 >= v["bytes"] / HBM_PEAK_GBS / 1e9 else "hbm",
                             **(pmc_sq(a.workload, k) if traffic is not None else {})}
                         for k, v in fam.items()}
            dom = max(fam, key=lambda k: fam[k]["ms"]) if fam else None
            if dom is not None:
                d = by_kernel[dom]
                dom_traffic, _ = (hbm_traffic(a.workload, max(alg_launches, 1), dom) if traffic is not None else (None, None))
                hbm_bound = d["bound"] == "hbm"
                # the same family in the committed rocprofv3 summary of this command: its kernel's name as rocprof prints it, and the
                # roofline fraction its average duration gives (the live HIP-event `frac` of THIS box beside it: boxes differ by 2-3 %)
                rp = rocprof_family(a.workload, dom, d["launches"]) if (world == 1 and not a.batch and not a.T and not a.chunk and a.dtype == "f16") else None
                per_launch = d["algorithmic_bytes_per_launch"] / 1e9 if hbm_bound else d["mfma_work_factor"] * d["algorithmic_flops_per_launch"] / 1e12
                line["roofline"] = {
                    "bound": d["bound"], "kernel": rp[0] if rp else dom, "kernel_family": dom,
                    "frac_rocprof": None if rp is None else round(per_launch / (rp[1] * 1e-3) / (HBM_PEAK_GBS if hbm_bound else MFMA_PEAK_TFLOPS), 4),
                    "avg_launch_ms_rocprof": None if rp is None else round(rp[1], 4), "rocprof_source": None if rp is None else rp[3],
                    "dominant_by": "hip_event_ms (the conv family with the most device time in the profiled step; "
                                                                       "quote whole_step.frac when comparing rounds)",
                    "rocprof_top_symbol": rocprof_top_symbol(a.workload) if rp else None,
                    "achieved": d["hbm_gbs_algorithmic"] if hbm_bound else d["achieved"],
                    "peak": HBM_PEAK_GBS if hbm_bound else d["peak_algorithmic_tflops"], "unit": "GB/s" if hbm_bound else "TFLOP/s",
                    "frac": d["hbm_frac"] if hbm_bound else d["frac"],
                    "traffic": None if dom_traffic is None else round(dom_traffic),
                    "traffic_unit": "fabric bytes per launch = L2 misses, Infinity-Cache hits included (PMC FETCH_SIZE x2 + WRITE_SIZE): an upper bound of the HBM bytes", "traffic_source": traffic_src,
                    "algorithmic_flops_per_launch": d["algorithmic_flops_per_launch"],
                    "algorithmic_bytes_per_launch": d["algorithmic_bytes_per_launch"],
                    "launches": d["launches"], "avg_launch_ms": d["avg_launch_ms"],
                    "share_of_step_ms": round(fam[dom]["ms"], 3),
                    "all_conv_launches": {"achieved": round(achieved, 2), "unit": "TFLOP/s", "frac": round(achieved / MFMA_PEAK_TFLOPS, 4),
                                          "launches": int(conv_launches), "avg_launch_ms": round(conv_ms / max(conv_launches, 1), 4),
                                          "traffic": None if traffic is None else round(traffic),
                                          "algorithmic_bytes_per_launch": round(alg_bytes / max(alg_launches, 1)),
                                          "algorithmic_flops_per_launch": round(conv_flops / max(conv_launches, 1))},
                    "whole_step": {"achieved": line["tflops_executed"], "unit": "TFLOP/s",
                                   "frac": round(line["tflops_executed"] / MFMA_PEAK_TFLOPS, 4)},
                    "by_kernel": by_kernel,
                    "profile_ms": {k: round(v[0], 3) for k, v in prof.items()}}
        if a.full and not a.no_cpu_baseline and world == 1:        # the CPU baseline is reported at N=1 only
            cpu_val, threads, cpu_mean, sweep = cpu_baseline(wl, B, a.cpu_T, a.seed)
            gpu_same = eng.predict(x, a.cpu_T, seed=a.seed)["mean"].cpu().numpy()
            other = "bf16" if a.dtype == "f16" else "f16"          # the other 16-bit instantiation (split engines: plain fp16) on the same inputs / masks
            eng_o = model.engine(dev, max_batch=B, chunk_samples=a.chunk or None, dtype=other)
            gpu_other = eng_o.predict(x, a.cpu_T, seed=a.seed)["mean"].cpu().numpy()
            one = cpu_baseline_1thread(wl, a.cpu_1t_images, 2, a.seed) if a.cpu_1t_images > 0 else None
            mp_val, mp_procs, mp_threads = cpu_baseline_multiproc(a, B, a.cpu_T, a.cpu_procs) if a.cpu_procs > 0 else (None, 0, 0)
            line["cpu_baseline"] = {
                "value": round(cpu_val, 1), "unit": "MCD-samples/s", "cores": threads, "kind": "port",
                "threads": threads, "cores_physical": physical_cores(), "logical_cpus": os.cpu_count(),
                "thread_sweep": {str(k): round(v, 1) for k, v in sweep.items()},
                "value_1thread": None if one is None else round(one, 2),
                "value_multiprocess": None if mp_val is None else round(mp_val, 1),
                "sample_multiprocess": f"the same loop as {mp_procs} processes x {mp_threads} threads over contiguous slices of the {B}-image batch, T={a.cpu_T}, all "
                                       f"warm before the clock starts, wall time until the last slice is done ({mp_procs * mp_threads} threads in use)",
                "sample_1thread": f"same oracle loop, torch.set_num_threads(1), {a.cpu_1t_images} images x T=2",
                "sample": f"oracle (port of FullAnalysis._get_output loop, ATen F.dropout as the RNG like the reference), 1 batch of {B} images x T={a.cpu_T}, fp32, "
                          f"torch {torch.__version__} CPU at its best intra-op thread count ({threads} of {os.cpu_count()} logical CPUs; "
                          f"thread_sweep = MCD-samples/s of 2 passes per candidate)",
                "ece_hist_final_exit_cpu": round(ece_hist_binary(cpu_mean[-1], onehot), 6),
                "ece_hist_final_exit_gpu_same_T": round(ece_hist_binary(gpu_same[-1], onehot), 6),
                "max_abs_mean_diff_gpu_vs_cpu": float(np.abs(gpu_same - cpu_mean).max()),
                f"max_abs_mean_diff_gpu_{other}_vs_cpu": float(np.abs(gpu_other - cpu_mean).max()),
            }
        if a.full and world == 1 and not a.no_parity_leg and a.dtype == "f16":
            line["parity"] = tolerance_leg(model, dev, x, B, T, a.seed, max(3, a.steps // 2), rec=auto_rec)
            line["parity_engine"] = line["parity"].get("parity_engine")
            line["value_at_tolerance"] = line["parity"].get("value_at_tolerance")
        if a.full and world == 1 and not a.no_rccl_probe:       # after everything timed: RCCL executed once on this GPU (SURVEY 8.5, round-4 review item 5)
            line["allreduce_us_1rank"] = rccl_probe_in_a_child(a)
        print(json.dumps(line), flush=True)
    if dist is not None:
        dist.barrier()
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
