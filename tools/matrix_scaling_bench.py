#!/usr/bin/env python3
"""Matrix scaling, measured.  One JSON line per measurement.

  (r) no GPU: the resource lines of the matrix-scaling head kernels beside their vector-scaling twins, and of ensemble.hip's twelve kernels
      (tools/kernel_resources.py);
  (a) the head launches and the ensemble launch under a matrix scaling against THE SAME ENGINE under a vector scaling, at the paper's size
      (exit-only dropout, B = 250, T = 10, C = 100) and at the headline size (block + exit dropout, B = 250, T = 100, C = 10): the engine's
      per-launch HIP events (bmi_profile_read's head slot) and HIP-event medians of the stand-alone ensemble entry on the same logits,
      alternating arms; the vector arm runs twice per round (A and A'), their spread is what a difference has to exceed;
  (b) one bmi_nll_matrix_scaling_grad launch against one bmi_nll_vector_scaling_grad launch on the same logits (B = 250, T = 10, E = 4,
      C = 100), and the whole MatrixScaling fit at N = 1 000 (off_diag_l2 = 1).

    python tools/matrix_scaling_bench.py [--rounds 9] [--launches 20] [--parts a,b]
    python tools/matrix_scaling_bench.py --parts r
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from vector_scaling_bench import SIZES, coeffs, event_ms, model_of, stats  # noqa: E402


def mat_coeffs(E, C, seed=0):
    """tests/test_matrix_scaling.py's coefficients: diagonal in [0.4, 2.2], bias in [-1, 1], off-diagonal U(-1, 1) * 0.3 / sqrt(C)."""
    rng = np.random.default_rng(300 + seed)
    M = rng.uniform(-1.0, 1.0, (E, C, C)) * 0.3 / np.sqrt(C)
    M[:, np.arange(C), np.arange(C)] = rng.uniform(0.4, 2.2, (E, C))
    return M.astype(np.float32), rng.uniform(-1.0, 1.0, (E, C)).astype(np.float32)


def part_r(a):
    import subprocess

    def table(src):
        out = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "kernel_resources.py"), src], capture_output=True, text=True)
        if out.returncode:
            sys.exit(out.stderr[-2000:])
        return {line[:90].strip(): line[90:].split() for line in out.stdout.splitlines()[1:]}
    vec, mat = table("head_fused_vec.hip"), table("head_fused_mat.hip")
    cols = ("sgpr", "vgpr", "agpr", "scratch", "occ", "s_spill", "v_spill", "lds")
    for name, v in mat.items():
        t = vec[name.replace("_mat_kernel", "_vec_kernel")]
        print(json.dumps(dict(part="r", kernel=name, **{c: int(x) for c, x in zip(cols, v)}, twin_vgpr=int(t[1]), twin_agpr=int(t[2]),
                              twin_occ=int(t[4]), twin_lds=int(t[7]))), flush=True)
    for name, v in table("ensemble.hip").items():
        if "ensemble_moments" in name:
            print(json.dumps(dict(part="r", kernel=name[:60], sgpr=int(v[0]), vgpr=int(v[1]), scratch=int(v[3]), occ=int(v[4]), v_spill=int(v[6]),
                                  lds=int(v[7]))), flush=True)
    for name, v in table("calibration.hip").items():
        if "nll_mat" in name or "nll_vec" in name:
            print(json.dumps(dict(part="r", kernel=name[:40], sgpr=int(v[0]), vgpr=int(v[1]), scratch=int(v[3]), occ=int(v[4]), v_spill=int(v[6]),
                                  lds=int(v[7]))), flush=True)


def part_a(a):
    from bayesnn_fpga_amd.synthetic import synthetic_images
    dev = torch.device("cuda", 0)
    for tag, (kw, B, T) in SIZES.items():
        m = model_of(kw, dev)
        eng = m.engine(dev, max_batch=B, dtype="f16")
        x = synthetic_images(B, seed=1234).to(dev)
        E, C = eng.n_exits, eng.out_dim
        va, vb = coeffs(E, C)
        mm, mb = mat_coeffs(E, C)

        def set_arm(k):
            if k.startswith("B"):
                eng.set_vector_scaling(None)
                eng.set_matrix_scaling(mm, mb)
            else:
                eng.set_matrix_scaling(None)
                eng.set_vector_scaling(va, vb)
        arms = ("A vector scaling", "B matrix scaling", "A' vector scaling")
        head = {k: [] for k in arms}
        step = {k: [] for k in arms}
        S = eng.new_moments(B)
        for k in arms:                                           # warm-up of both instantiations
            set_arm(k)
            eng.accumulate(x, S, 0, T, 1)
        torch.cuda.synchronize()
        for r in range(a.rounds):
            for k in (arms if r % 2 == 0 else arms[::-1]):
                set_arm(k)
                step[k].append(event_ms(lambda: eng.accumulate(x, S, 0, T, 1), 3))
                eng.profile(True)
                eng.accumulate(x, S, 0, T, 1)
                ms, n = eng.profile_read()["head"]
                eng.profile(False)
                head[k].append(ms)
        groups = B * ((T + 31) // 32) * E
        for k in arms:
            print(json.dumps(dict(part="a", size=tag, what="head launches of one step, summed (per-launch HIP events)", arm=k, B=B, T=T, C=C,
                                  launches=int(n), workgroups=groups, **stats(head[k]),
                                  ratio_to_A=round(stats(head[k])["median_ms"] / stats(head[arms[0]])["median_ms"], 4))), flush=True)
        for k in arms:
            print(json.dumps(dict(part="a", size=tag, what="accumulate, one step end to end", arm=k, B=B, T=T, C=C, **stats(step[k]),
                                  ratio_to_A=round(stats(step[k])["median_ms"] / stats(step[arms[0]])["median_ms"], 4))), flush=True)
        eng.set_vector_scaling(None)
        eng.set_matrix_scaling(None)
        # the ensemble launch on the same logits, straight through the C ABI
        logits = eng.forward_samples(x, T, seed=1)
        Q = torch.zeros(2, E, B, C, dtype=torch.float64, device=dev)
        QH = torch.zeros(E, B, dtype=torch.float64, device=dev)
        ad, bd = torch.from_numpy(va).to(dev), torch.from_numpy(vb).to(dev)
        md, mbd = torch.from_numpy(mm).to(dev), torch.from_numpy(mb).to(dev)
        lib, st = eng.lib, eng._stream()

        def vector():
            return lib.bmi_ensemble_moments_vector(logits.data_ptr(), T, E, B, C, ad.data_ptr(), bd.data_ptr(), None, Q[0].data_ptr(), Q[1].data_ptr(),
                                                   QH.data_ptr(), st)

        def matrix():
            return lib.bmi_ensemble_moments_matrix(logits.data_ptr(), T, E, B, C, md.data_ptr(), mbd.data_ptr(), None, Q[0].data_ptr(), Q[1].data_ptr(),
                                                   QH.data_ptr(), st)
        assert vector() == 0 and matrix() == 0
        fns = {arms[0]: vector, arms[1]: matrix, arms[2]: vector}
        times = {k: [] for k in arms}
        for fn in fns.values():
            for _ in range(5):
                fn()
        torch.cuda.synchronize()
        for r in range(a.rounds):
            for k in (arms if r % 2 == 0 else arms[::-1]):
                times[k].append(event_ms(fns[k], a.launches))
        for k in arms:
            s = stats(times[k])
            print(json.dumps(dict(part="a", size=tag, what="ensemble launch", arm=k, B=B, T=T, E=E, C=C, launches_per_timing=a.launches,
                                  timings=a.rounds, **s, ratio_to_A=round(s["median_ms"] / stats(times[arms[0]])["median_ms"], 4))), flush=True)


def banded_teacher_problem(dev, N, Bb, T, seed, C=100):
    """tests/test_matrix_scaling.py's teacher-label model: labels drawn from softmax(M* mean logits), M* banded and not diagonal."""
    from bayesnn_fpga_amd.synthetic import synthetic_images
    m = model_of(dict(dropout_exit=True, dropout=None, dropout_p=0.25, out_dim=C), dev)
    m.engine_dtype = "f16x2"
    x = synthetic_images(N, seed=31)
    eng = m.engine(dev, max_batch=Bb)
    nb = N // Bb
    raw = np.concatenate([eng.forward_samples(x[k * Bb:(k + 1) * Bb].to(dev), T, seed=seed + k).cpu().numpy() for k in range(nb)], axis=2)
    rng = np.random.default_rng(7)
    Ms = np.eye(C) * 1.5
    for c in range(C):
        Ms[c, (c + 1) % C], Ms[c, (c - 1) % C] = 0.9, -0.4
    z = raw.mean(0)[-1].astype(np.float64) @ Ms.T
    p = np.exp(z - z.max(-1, keepdims=True))
    labels = np.array([rng.choice(C, p=q / q.sum()) for q in p])
    y = torch.from_numpy(labels)
    return m, raw, labels, [(x[k * Bb:(k + 1) * Bb], y[k * Bb:(k + 1) * Bb]) for k in range(nb)]


def part_b(a):
    from bayesnn_fpga_amd.train.calibration import MatrixScaling
    dev = torch.device("cuda", 0)
    B, T, E, C = 250, 10, 4, 100
    m, raw, labels, loader = banded_teacher_problem(dev, 1000, B, T, 5)
    eng = m.engine(dev, max_batch=B)
    logits = torch.from_numpy(np.ascontiguousarray(raw[:, :, :B])).to(dev)
    y_dev = torch.from_numpy(labels[:B]).to(dev, torch.int32)
    va, vb = coeffs(E, C)
    mm, mb = mat_coeffs(E, C)
    a64, b64 = torch.from_numpy(va.astype(np.float64)).to(dev), torch.from_numpy(vb.astype(np.float64)).to(dev)
    m64, mb64 = torch.from_numpy(mm.astype(np.float64)).to(dev), torch.from_numpy(mb.astype(np.float64)).to(dev)
    out_v = eng.nll_vector_grad(logits, y_dev, a64, b64)
    out_m = eng.nll_matrix_grad(logits, y_dev, m64, mb64)
    fns = {"A nll_vector_grad launch": lambda: eng.nll_vector_grad(logits, y_dev, a64, b64, out=out_v),
           "B nll_matrix_grad launch": lambda: eng.nll_matrix_grad(logits, y_dev, m64, mb64, out=out_m),
           "A' nll_vector_grad launch": lambda: eng.nll_vector_grad(logits, y_dev, a64, b64, out=out_v)}
    arms = list(fns)
    times = {k: [] for k in arms}
    for fn in fns.values():
        for _ in range(5):
            fn()
    torch.cuda.synchronize()
    for r in range(a.rounds):
        for k in (arms if r % 2 == 0 else arms[::-1]):
            times[k].append(event_ms(fns[k], a.launches))
    for k in arms:
        s = stats(times[k])
        print(json.dumps(dict(part="b", what=k + " (two kernels each, through MCDEngine)", B=B, T=T, E=E, C=C, **s,
                              ratio_to_A=round(s["median_ms"] / stats(times[arms[0]])["median_ms"], 4))), flush=True)
    ms = MatrixScaling(m, loader, gpu=0, mc_passes=T, seed=5)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    r = ms.fit(off_diag_l2=1.0, max_iter=a.max_iter)
    torch.cuda.synchronize()
    t1 = time.perf_counter()
    print(json.dumps(dict(part="b", what="MatrixScaling.fit, whole (walk + vector fit + L-BFGS on the matrix), host clock", n=r["n"],
                          max_iter=a.max_iter, off_diag_l2=1.0, fit_s=round(t1 - t0, 3), iterations=[int(i) for i in r["iterations"]],
                          converged=[bool(c) for c in r["converged"]], nll_start=[round(float(v), 3) for v in r["nll_start"]],
                          nll_after=[round(float(v), 3) for v in r["nll_after"]], penalty=[round(float(v), 3) for v in r["penalty"]])), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--launches", type=int, default=20)
    ap.add_argument("--max-iter", type=int, default=50)
    ap.add_argument("--parts", default="a,b")
    a = ap.parse_args()
    parts = a.parts.split(",")
    if set(parts) - {"r"} and not torch.cuda.is_available():
        sys.exit("matrix_scaling_bench.py measures parts a and b on the GPU: none visible (--parts r needs none)")
    for p in parts:
        {"r": part_r, "a": part_a, "b": part_b}[p](a)


if __name__ == "__main__":
    main()
