"""The detection read-out without a GPU: ``detection_metrics(rank_detection_numpy(...))`` against the plain definitions in exact rational
arithmetic — every distinct key as a threshold, its TP / FP / precision / recall, AP = sum of (recall step) * precision, and the smallest
FPR among the thresholds whose TPR reaches q — on hand-sized rows with ties across the classes."""
from fractions import Fraction

import numpy as np
import pytest

from bayesnn_fpga_amd.train.ranking import INVALID, detection_metrics, rank_detection_numpy, rank_quality_numpy

TPR = (0.25, 0.5, 0.95, 1.0)
CASES = {
    "ties across the classes": ([3, 1, 3, 2, 2, 3, 1, 1, 2, 3, 5, 5], [1, 0, 0, 1, 0, 1, 0, 0, 1, 1, 0, 1]),
    "two keys, forty images": ([7, 9] * 20, [0, 0, 1, 0, 1, 1, 0, 1] * 5),
    "an invalid image, distinct and tied keys": ([10, INVALID, 11, 12, 12, 12, 13, 14, INVALID, 14], [0, 1, 0, 1, 0, 1, 1, 0, 0, 1]),
    "one key": ([4] * 9, [1, 0, 0, 1, 0, 0, 0, 1, 0]),
    "no negative": ([1, 2, 2, 3], [1, 1, 1, 1]),
}


def plain(keys, positive):
    """(AP of "key >= t flags a positive", AP of "key <= t flags a negative", the smallest FPR with TPR >= q per level): Fractions, None
    where the class divided by is empty"""
    pairs = [(k, p) for k, p in zip(keys, positive) if k != INVALID]
    n_pos = sum(p for _, p in pairs)
    n_neg = len(pairs) - n_pos
    levels = sorted({k for k, _ in pairs})
    ap_pos = ap_neg = None
    points = []
    if n_pos:
        ap_pos, recall = Fraction(0), Fraction(0)
        for t in reversed(levels):
            tp = sum(p for k, p in pairs if k >= t)
            fp = sum(1 - p for k, p in pairs if k >= t)
            ap_pos += (Fraction(tp, n_pos) - recall) * Fraction(tp, tp + fp)
            recall = Fraction(tp, n_pos)
            points.append((recall, fp))
    if n_neg:
        ap_neg, recall = Fraction(0), Fraction(0)
        for t in levels:
            tn = sum(1 - p for k, p in pairs if k <= t)
            flagged = sum(1 for k, _ in pairs if k <= t)
            ap_neg += (Fraction(tn, n_neg) - recall) * Fraction(tn, flagged)
            recall = Fraction(tn, n_neg)
    fpr = [Fraction(min(fp for rec, fp in points if rec >= Fraction(q)), n_neg) if n_pos and n_neg else None for q in TPR]
    return ap_pos, ap_neg, fpr


@pytest.mark.parametrize("case", sorted(CASES))
def test_detection_metrics_equal_the_plain_definitions(case):
    keys, positive = CASES[case]
    u, p = np.array([keys], dtype=np.uint32), np.array([positive], dtype=np.uint8)
    table = rank_quality_numpy(u, p, len(keys))
    det = rank_detection_numpy(table, TPR)
    got = detection_metrics(det, table)
    n_neg = int(table["counts"][0, 0] - table["counts"][0, 1])
    ap_pos, ap_neg, fpr = plain(keys, positive)
    bound = (int(table["counts"][0, 0]) + 2) * 2.0 ** -53    # m non-negative terms, each one division and one addition, each rounded once
    for name, want in (("aupr_pos", ap_pos), ("aupr_neg", ap_neg)):
        if want is None:
            assert np.isnan(got[name][0]), name
        else:
            assert abs(Fraction(float(got[name][0])) - want) <= Fraction(bound) * want, (name, float(got[name][0]), float(want))
    for l, want in enumerate(fpr):
        if want is None:
            assert np.isnan(got["fpr_at_tpr"][0, l])
        else:
            assert Fraction(int(det["det"][0, l, 1]), n_neg) == want and got["fpr_at_tpr"][0, l] == int(det["det"][0, l, 1]) / n_neg, (TPR[l], want)
