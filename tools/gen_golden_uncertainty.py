#!/usr/bin/env python3
"""Generate tests/golden/uncertainty_ape.npz with THE REFERENCE'S OWN aPE function.

Runs only in the build container (needs the reference checkout; never on the GPU box).  The reference's
Hardware_Artifact/bayes_hw/metric_utils.py (numpy only) is imported from where it lies, never copied; only the
probability sets and what its ``entropy()`` returns for them are written:

    PYTHONDONTWRITEBYTECODE=1 python tools/gen_golden_uncertainty.py

Keys: ``p_<name>`` (float64 [N, C] probabilities) and ``ape_<name>`` (the reference's entropy() of that set), for
  * ``metrics``          — the ``p`` of tests/golden/metrics.npz;
  * ``peaky``            — rows with exact zeros: one-hots, two-way ties, softmaxes of logits scaled until most classes underflow;
  * ``c100_exit<e>``     — the T-mean softmax of exit e of the resnet18_mask8_exit_c100 golden's per-pass logits (float64).
"""
import importlib.util
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = "/root/reference/Hardware_Artifact/bayes_hw/metric_utils.py"
GOLDEN = os.path.join(REPO, "tests", "golden")
sys.dont_write_bytecode = True


def _ref_entropy():
    spec = importlib.util.spec_from_file_location("ref_metric_utils", REF)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod.entropy


def softmax64(logits):
    z = np.asarray(logits, dtype=np.float64)
    z = z - z.max(axis=-1, keepdims=True)
    e = np.exp(z)
    return e / e.sum(axis=-1, keepdims=True)


def peaky_set(seed=0):
    rng = np.random.default_rng(seed)
    C = 10
    rows = [np.eye(C)[c] for c in range(C)]                       # one-hots: entropy 0, every other entry an exact zero
    tie = np.zeros(C)
    tie[[2, 7]] = 0.5
    rows.append(tie)
    for scale in (50.0, 200.0, 1000.0):                            # softmax in float64 until exp() underflows to exact zeros
        rows.extend(softmax64(rng.standard_normal((8, C)) * scale))
    p = np.stack(rows)
    assert (p == 0).any(axis=1).sum() >= C
    return p


def main():
    entropy = _ref_entropy()
    sets = {"metrics": np.load(os.path.join(GOLDEN, "metrics.npz"))["p"].astype(np.float64), "peaky": peaky_set()}
    g = np.load(os.path.join(GOLDEN, "resnet18_mask8_exit_c100.npz"), allow_pickle=True)
    mean = softmax64(g["logits"]).mean(axis=0)                      # [T, E, B, C] -> [E, B, C]
    for e in range(mean.shape[0]):
        sets[f"c100_exit{e}"] = mean[e]
    out = {}
    for name, p in sets.items():
        out[f"p_{name}"] = p
        out[f"ape_{name}"] = np.float64(entropy(p))
    path = os.path.join(GOLDEN, "uncertainty_ape.npz")
    np.savez(path, **out)
    print(path, {k: (v.shape, float(v) if v.ndim == 0 else None) for k, v in out.items()})


if __name__ == "__main__":
    main()
