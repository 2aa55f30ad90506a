"""Reliability tables over a loader: per exit and per exit ensemble the confidence histogram behind the top-label ECE (the equal-mass bins
of ``train.metrics.ece_hist_binary``, SA/train/results_analyzer.py:446-495, or equal-width ones), the NLL and the Brier score (the
reference's "MSE", :497-503) — the ``ECE, NLL, MSE`` columns of ``FullAnalysis.all_experiments``, formed on the device
(csrc/reliability.hip: ``MCDEngine.reliability_records`` per batch, ONE ``MCDEngine.reliability_table`` at the end) from integer-exact tables.

``reliability_numpy`` restates the device's arithmetic contract (the header comment of csrc/reliability.hip) on the host, loop by loop;
``table_metrics`` derives the metrics from a table, the device's or the restatement's.
"""
import numpy as np

from .results_analyzer import get_device

FIX = 2.0 ** 40           # conf_fix counts confidences in units of 2^-40


def _np(a):
    return a.detach().cpu().numpy() if hasattr(a, "detach") else np.asarray(a)


def width_edges(n_bins):
    """edges[i] = (float) i / n_bins, float32 [n_bins + 1]"""
    return (np.arange(n_bins + 1, dtype=np.float32) / np.float32(n_bins)).astype(np.float32)


INVALID = np.uint32(0xFFFFFFFF)   # a classwise key of a (row, image) that is not data (ranking.hip's convention)
FLUSH = 2.0 ** -126               # a quotient below the least normal float32 is confidence zero


def _record_rows(mean, labels, binnings, binning):
    """What both restatements do before they differ.  Checks the arguments; returns ((E, N, C), y int64 [N], labelled bool [N], rows): ``rows``
    yields per row r = kind * E + e the tuple (valid bool [N] — labelled and every v_c finite —, the labelled images with a non-finite
    v_c, v [N, C] — 1.0, a finite placeholder whose results are dropped, where not valid —, pc = max(v, 1e-256), s [N] = the class sum
    as an explicit ascending loop)."""
    mean = np.asarray(mean, dtype=np.float64)
    if mean.ndim != 3:
        raise ValueError("mean must be [E, N, C]")
    E, N, Cd = mean.shape
    y = np.asarray(labels).astype(np.int64).reshape(-1)
    if y.shape[0] != N:
        raise ValueError("labels must be [N]")
    if binning not in binnings:
        raise ValueError("binning must be " + ", ".join(repr(b) for b in binnings[:-1]) + f" or {binnings[-1]!r}, got {binning!r}")
    labelled = (y >= 0) & (y < Cd)

    def rows():
        acc = np.zeros((N, Cd), dtype=np.float64)
        with np.errstate(invalid="ignore", over="ignore"):
            per_exit = []
            for e in range(E):
                acc = acc + mean[e]
                per_exit.append(acc / float(e + 1))
        for v in list(mean) + per_exit:
            finite = np.isfinite(v).all(axis=1)
            valid = labelled & finite
            v = np.where(valid[:, None], v, 1.0)
            pc = np.maximum(v, 1e-256)
            s = np.zeros(N, dtype=np.float64)
            for c in range(Cd):                              # ascending class order
                s = s + pc[:, c]
            yield valid, int((labelled & ~finite).sum()), v, pc, s
    return (E, N, Cd), y, labelled, rows()


def _mass_edges(line, n_bins):
    """float32 [n_bins + 1]: the equal-mass edges of one line of N uint32 keys — 0, the order statistics of rank min((i + 1) * per, N - 1),
    per = N // n_bins, in unsigned key order (the float order of the confidences; INVALID keys last, a selected one is the edge 1.0), 1."""
    N = line.shape[0]
    per = N // n_bins
    srt = np.sort(line)
    out = np.empty(n_bins + 1, dtype=np.float32)
    out[0] = 0.0
    for i in range(n_bins):
        k = srt[min((i + 1) * per, N - 1)]
        out[i + 1] = 1.0 if k == INVALID else k.view(np.float32)
    out[n_bins] = 1.0
    return out


def reliability_numpy(mean, labels, n_bins=15, binning="mass"):
    """The host restatement of bmi_reliability_record + bmi_reliability_table: ``mean`` float64 [E, N, C] (T-mean probabilities), ``labels``
    int [N].  Rows r = kind * E + e: the exits (kind 0), then the exit ensembles (p_0 + ... + p_e) / (e + 1), added in exit order and divided
    once.  Returns dict(keys uint32, hit uint8, nll, brier float64 [R, N] — the records —, edges float32 [R, n_bins + 1], count, hits,
    conf_fix int64 [R, n_bins], nll_sum, brier_sum float64 [R], nonfinite, badlabel, n).  Every sum is an explicit ascending loop: over
    the classes for a row's probability sum and Brier term, over the images for the two float64 sums."""
    (E, N, _), y, labelled, rows = _record_rows(mean, labels, ("mass", "width"), binning)
    n_bins = int(n_bins)
    R = 2 * E
    yy = np.where(labelled, y, 0)
    keys = np.zeros((R, N), dtype=np.uint32)
    hit = np.zeros((R, N), dtype=np.uint8)
    nll = np.zeros((R, N), dtype=np.float64)
    brier = np.zeros((R, N), dtype=np.float64)
    nonfinite = 0
    idx = np.arange(N)
    for r, (valid, bad, v, pc, s) in enumerate(rows):
        nonfinite += bad
        b = np.zeros(N, dtype=np.float64)
        for c in range(v.shape[1]):                          # ascending class order
            d = v[:, c] - (yy == c)
            b = b + d * d
        pred = pc.argmax(axis=1)                             # numpy's argmax: the lowest index on ties
        conf = (pc[idx, pred] / s).astype(np.float32)
        keys[r] = np.where(valid, conf.view(np.uint32), 0)
        hit[r] = valid & (pred == yy)
        nll[r] = np.where(valid, -np.log(pc[idx, yy]), 0.0)
        brier[r] = np.where(valid, b, 0.0)
    edges = np.empty((R, n_bins + 1), dtype=np.float32)
    for r in range(R):
        edges[r] = _mass_edges(keys[r], n_bins) if binning == "mass" else width_edges(n_bins)
    count = np.zeros((R, n_bins), dtype=np.int64)
    hits = np.zeros((R, n_bins), dtype=np.int64)
    conf_fix = np.zeros((R, n_bins), dtype=np.int64)
    nll_sum = np.zeros(R, dtype=np.float64)
    brier_sum = np.zeros(R, dtype=np.float64)
    for r in range(R):
        conf = keys[r].view(np.float32)
        for i in range(n_bins):
            sel = (keys[r] != 0) & (conf > edges[r, i]) & (conf <= edges[r, i + 1])
            count[r, i] = int(sel.sum())
            hits[r, i] = int(hit[r][sel].sum())
            conf_fix[r, i] = int((conf[sel].astype(np.float64) * FIX).astype(np.int64).sum())
        s = t = 0.0
        for a, b in zip(nll[r].tolist(), brier[r].tolist()):  # image order
            s = s + a
            t = t + b
        nll_sum[r], brier_sum[r] = s, t
    return dict(keys=keys, hit=hit, nll=nll, brier=brier, edges=edges, count=count, hits=hits, conf_fix=conf_fix, nll_sum=nll_sum,
                brier_sum=brier_sum, nonfinite=nonfinite, badlabel=int((~labelled).sum()), n=N)


def table_metrics(table, n=None):
    """float64 on the host, from a table of ``MCDEngine.reliability_table`` or ``reliability_numpy`` (``n``: the number of images, default
    ``table['n']``): dict(acc, ece, mce, nll, brier), each [R].  ece = sum_i |conf_fix_i / 2^40 / count_i - hits_i / count_i| * count_i / n
    over the non-empty bins in bin order, mce the largest such gap, nll = nll_sum / n, brier = brier_sum / n, acc = sum_i hits_i / n."""
    n = int(table["n"] if n is None else n)
    count, hits, fix = (_np(table[k]).astype(np.int64) for k in ("count", "hits", "conf_fix"))
    R, n_bins = count.shape
    ece = np.zeros(R, dtype=np.float64)
    mce = np.zeros(R, dtype=np.float64)
    for r in range(R):
        for i in range(n_bins):
            k = int(count[r, i])
            if k == 0:
                continue
            gap = abs(float(fix[r, i]) / FIX / k - float(hits[r, i]) / k)
            ece[r] = ece[r] + gap * k / n
            mce[r] = max(mce[r], gap)
    return dict(acc=hits.sum(axis=1) / float(n), ece=ece, mce=mce, nll=_np(table["nll_sum"]).astype(np.float64) / n,
                brier=_np(table["brier_sum"]).astype(np.float64) / n)


def classwise_numpy(mean, labels, n_bins=15, binning="width", edges=None):
    """The host restatement of bmi_classwise_record + bmi_classwise_table (the header comment of csrc/reliability_classwise.hip): ``mean``
    float64 [E, N, C], ``labels`` int [N]; rows r = kind * E + e as in ``reliability_numpy``.  Per (row, image): pc = max(v, 1e-256), s the
    ascending class sum, and for EVERY class conf_c = 0.0f if pc_c / s < 2^-126 else (float) (pc_c / s).  ``binning``: "width" (``width_edges(
    n_bins)``: the published classwise ECE), "mass" (per (row, class) the order statistics of its N keys) or "edges" (the caller's ``edges``
    float32 [n_bins + 1], which then sets ``n_bins``).  Bin 0 is closed at its lower edge: confidence zero is counted.

    Returns dict(pkeys uint32 [R, C, N] — INVALID (all ones) where the label is outside [0, C) or the row non-finite —, labels int32 [N]
    (-1 for a bad label), edges float32 [R, C, n_bins + 1], count, hits, conf_fix int64 [R, C, n_bins] (conf_fix = sum of the TRUNCATED
    (int64) (conf * 2^40)), valid int64 [R], nonfinite, badlabel, n).  4 R C bytes per image on the device.  The class sum is an explicit
    ascending loop; the rest loops over rows and bins and is vectorised over classes and images (integer sums: order-free)."""
    (E, N, Cd), y, labelled, rows = _record_rows(mean, labels, ("mass", "width", "edges"), binning)
    if binning == "edges":
        if edges is None:
            raise ValueError("binning 'edges' needs edges [n_bins + 1]")
        fixed = np.asarray(edges, dtype=np.float32).reshape(-1)
        n_bins = fixed.shape[0] - 1
        if n_bins < 1 or not np.isfinite(fixed).all() or (np.diff(fixed) < 0).any():
            raise ValueError("edges must be finite, non-decreasing and at least two")
    else:
        n_bins = int(n_bins)
        fixed = width_edges(n_bins) if binning == "width" else None
    R = 2 * E
    pkeys = np.empty((R, Cd, N), dtype=np.uint32)
    valid = np.zeros(R, dtype=np.int64)
    nonfinite = 0
    for r, (ok, bad, _, pc, s) in enumerate(rows):
        nonfinite += bad
        valid[r] = int(ok.sum())
        for c in range(Cd):
            q = pc[:, c] / s
            conf = np.where(q < FLUSH, 0.0, q).astype(np.float32)
            pkeys[r, c] = np.where(ok, conf.view(np.uint32), INVALID)
    out_edges = np.empty((R, Cd, n_bins + 1), dtype=np.float32)
    for r in range(R):
        for c in range(Cd):
            out_edges[r, c] = _mass_edges(pkeys[r, c], n_bins) if fixed is None else fixed
    count = np.zeros((R, Cd, n_bins), dtype=np.int64)
    hits = np.zeros((R, Cd, n_bins), dtype=np.int64)
    conf_fix = np.zeros((R, Cd, n_bins), dtype=np.int64)
    is_label = (np.where(labelled, y, -1)[None, :] == np.arange(Cd)[:, None])               # [C, N]
    for r in range(R):
        data = pkeys[r] != INVALID
        conf = np.where(data, pkeys[r], 0).astype(np.uint32).view(np.float32)               # [C, N]
        fix = (conf.astype(np.float64) * FIX).astype(np.int64)                              # truncates
        ed = out_edges[r]
        for i in range(n_bins):
            lower = conf >= ed[:, 0, None] if i == 0 else conf > ed[:, i, None]
            sel = data & lower & (conf <= ed[:, i + 1, None])  # (the edges do not decrease: above edges[i] is at or above edges[0])
            count[r, :, i] = sel.sum(axis=1)
            hits[r, :, i] = (sel & is_label).sum(axis=1)
            conf_fix[r, :, i] = np.where(sel, fix, 0).sum(axis=1)
    return dict(pkeys=pkeys, labels=np.where(labelled, y, -1).astype(np.int32), edges=out_edges, count=count, hits=hits, conf_fix=conf_fix,
                valid=valid, nonfinite=nonfinite, badlabel=int((~labelled).sum()), n=N)


def classwise_metrics(table):
    """float64 on the host, from a table of ``MCDEngine.classwise_table`` or ``classwise_numpy``: dict(cw_ece_per_class [R, C] =
    sum_i |hits_i - conf_fix_i / 2^40| / valid[r] — class c's share of the classwise ECE: per bin |accuracy - mean confidence| weighted by
    count / valid —, cw_ece [R] = its mean over the classes, cw_mce [R, C] = the largest |hits_i / count_i - conf_fix_i / 2^40 / count_i|
    over the non-empty bins, class_count int64 [R, C] = sum_i hits_i (the valid images of label c that a bin holds)).  A row with
    ``valid == 0`` gives NaN."""
    count, hits, fix, valid = (_np(table[k]).astype(np.int64) for k in ("count", "hits", "conf_fix", "valid"))
    R, Cd, n_bins = count.shape
    per_class = np.full((R, Cd), np.nan, dtype=np.float64)
    mce = np.full((R, Cd), np.nan, dtype=np.float64)
    for r in range(R):
        if valid[r] == 0:
            continue
        gap = np.abs(hits[r].astype(np.float64) - fix[r].astype(np.float64) / FIX)           # [C, n_bins]
        tot = np.zeros(Cd, dtype=np.float64)
        for i in range(n_bins):                              # bin order
            tot = tot + gap[:, i]
        per_class[r] = tot / float(valid[r])
        filled = count[r] > 0
        k = np.where(filled, count[r], 1).astype(np.float64)
        mce[r] = np.where(filled, np.abs(hits[r] / k - fix[r].astype(np.float64) / FIX / k), 0.0).max(axis=1)
    return dict(cw_ece=per_class.mean(axis=1), cw_ece_per_class=per_class, cw_mce=mce, class_count=hits.sum(axis=2))


def kde_bw_scale(n):
    """The reference's bandwidth factor (2 N)^-0.2 (SA/train/results_analyzer.py:386-391), formed on the host: what ``reliability_kde``
    receives as ``bw_scale`` by default"""
    return float(2 * int(n)) ** -0.2


def reliability_kde_numpy(keys, hit, n, grid_points=2 ** 14, order=1, bw_scale=None):
    """The host restatement of bmi_reliability_kde (the header comment of csrc/reliability_kde.hip): the top-label KDE-ECE of
    ``train.metrics.ece_kde_binary`` — the reference's ``ECE`` — from the records' ``keys`` (uint32 or int32 [R, capacity]: the float32
    confidences' bit patterns) and ``hit`` (uint8 [R, capacity]), columns ``0 .. n - 1``, with the exact (un-binned) triweight densities.
    Float64 throughout; the sums over the images (mean, squared deviations, the density sums S1 and S2) are explicit loops in image order,
    vectorised over the grid only; a centre adds to the grid points around it alone (the others would receive +0.0); the carry-forward and
    the two trapezoids are explicit loops in index order.  ``bw_scale``: default ``kde_bw_scale(n)``.

    Two differences from ``ece_kde_binary`` are on purpose: the records hold the FLOAT32 confidence, which is used for both densities (the
    host function uses the unrounded float64 quotient for the density of all confidences), and the standard deviation is the float64
    two-pass sum of the contract, not ``np.std`` of a float32 array.  A row with no data or a zero denominator (no hit, one hit, equal hit
    confidences: the host function's NaN) is ``degenerate``: flag 1, value 0.0.

    Returns dict(ece_kde, bw, sd float64 [R], n_data, n_hit int64 [R], degenerate int32 [R], density float64 [R, 2, G] = pp1, pp2 — the
    device's outputs —, and the intermediates x [G], sums [R, 2, G] = S1, S2, h, perc, a, b [R], integrand [R, G], is_set [R, G] (the
    integrand was formed there, not carried), mirror_high [R, n] (the datum's mirror is 2 - d))."""
    import math
    keys = np.ascontiguousarray(_np(keys))
    if keys.dtype == np.int32:
        keys = keys.view(np.uint32)
    hit = np.asarray(_np(hit))
    n, G, order = int(n), int(grid_points), int(order)
    scale = kde_bw_scale(n) if bw_scale is None else float(bw_scale)
    if keys.dtype != np.uint32 or keys.ndim != 2 or hit.shape != keys.shape or not 1 <= n <= keys.shape[1]:
        raise ValueError("keys uint32 / int32 [R, capacity], hit [R, capacity], 1 <= n <= capacity")
    if not 16 <= G <= 65536 or order not in (1, 2) or not 2.0 ** -100 <= scale <= 2.0 ** 100:
        raise ValueError("grid_points in [16, 65536], order 1 or 2, bw_scale in [2^-100, 2^100]")
    R = keys.shape[0]
    step = 2.2 / float(G - 1)
    x = np.arange(G, dtype=np.float64) * step + (-0.6)
    inside = (x > 0.0) & (x < 1.0)
    in_range = np.nonzero((x >= 0.0) & (x <= 1.0))[0]
    out = dict(ece_kde=np.zeros(R), bw=np.zeros(R), sd=np.zeros(R), n_data=np.zeros(R, dtype=np.int64), n_hit=np.zeros(R, dtype=np.int64),
               degenerate=np.zeros(R, dtype=np.int32), density=np.zeros((R, 2, G)), x=x, sums=np.zeros((R, 2, G)), h=np.zeros(R),
               perc=np.zeros(R), a=np.zeros(R), b=np.zeros(R), integrand=np.zeros((R, G)), is_set=np.zeros((R, G), dtype=bool),
               mirror_high=np.zeros((R, n), dtype=bool))
    for r in range(R):
        data = keys[r, :n] != 0
        d_all = keys[r, :n].view(np.float32).astype(np.float64)
        is_hit = data & (hit[r, :n] != 0)
        nd, n1 = int(data.sum()), int(is_hit.sum())
        s = q = sd = 0.0
        if n1:
            for d in d_all[is_hit].tolist():                 # image order
                s = s + d
            mu = s / float(n1)
            for d in d_all[is_hit].tolist():
                q = q + (d - mu) * (d - mu)
            sd = math.sqrt(q / float(n1))
        bw = (sd if sd != 0.0 else 1e-16) * scale
        h = 3.0 * bw
        S = out["sums"][r]
        for d, hd in zip(d_all[data].tolist(), is_hit[data].tolist()):           # image order
            for c in (d, -d if d < 0.5 else 2.0 - d):
                # the grid points within h of the centre, one to spare on either side: every other term is nothing
                lo = max(int(np.searchsorted(x, c - h)) - 1, 0)
                hi = min(int(np.searchsorted(x, c + h)) + 1, G)
                u = (x[lo:hi] - c) / h
                t = 1.0 - u * u
                term = np.where(t > 0.0, t * t * t, 0.0)
                S[1, lo:hi] = S[1, lo:hi] + term
                if hd:
                    S[0, lo:hi] = S[0, lo:hi] + term
        out["mirror_high"][r] = data & ~(d_all < 0.5)
        pp1 = np.where(inside, S[0] * (35.0 / 32.0) / (h * float(2 * n1)) * 2.0, 0.0) if n1 else np.zeros(G)
        pp2 = np.where(inside, S[1] * (35.0 / 32.0) / (h * float(2 * nd)) * 2.0, 0.0) if nd else np.zeros(G)
        perc = float(n1) / float(nd) if nd else 0.0
        is_set = np.maximum(pp1, pp2) > 1e-6
        with np.errstate(divide="ignore", invalid="ignore"):
            e = np.abs(x - np.minimum(perc * pp1 / pp2, 1.0))
        formed = (e * e if order == 2 else e) * pp2
        I = np.zeros(G)
        for i in range(G):                                   # index order: the carry-forward is sequential
            if is_set[i]:
                I[i] = formed[i]
            elif i >= 2:
                I[i] = I[i - 1]
        a = b = 0.0
        for i in in_range[:-1].tolist():                     # (the indices in [0, 1] are consecutive)
            a = a + (x[i + 1] - x[i]) * (I[i + 1] + I[i]) / 2.0
            b = b + (x[i + 1] - x[i]) * (pp2[i + 1] + pp2[i]) / 2.0
        deg = nd == 0 or b == 0.0
        out["ece_kde"][r] = 0.0 if deg else a / b
        for k, v in (("bw", bw), ("sd", sd), ("n_data", nd), ("n_hit", n1), ("degenerate", int(deg)), ("h", h), ("perc", perc), ("a", a), ("b", b)):
            out[k][r] = v
        out["density"][r, 0], out["density"][r, 1] = pp1, pp2
        out["integrand"][r], out["is_set"][r] = I, is_set
    return out


def row_names(n_exits):
    """The row labels of ``FullAnalysis.all_experiments``: the exits "0", "1", ..., then "Ensemble0", "Ensemble1", ..."""
    return [str(e) for e in range(n_exits)] + [f"Ensemble{e}" for e in range(n_exits)]


class ReliabilityAnalysis:
    """One walk of ``loader`` (batches ``(x, y, ...)``) with ``mc_passes`` stochastic passes per batch, the calibration metrics formed on the
    device.  The walk is ``UncertaintyAnalysis``'s: batch k runs under seed ``seed + k`` with the model's current Masksembles counter, the
    counters advance by ``mc_passes`` afterwards (``model.advance``), the engine is the model's (``engine_dtype="auto"`` applies) — so the
    T-mean probabilities are ``FullAnalysis(model, loader, mc_dropout=True, mc_passes=T, seed=seed).preds``.  Per batch only the records
    (``MCDEngine.reliability_records``: 21 bytes per row and image) stay on the device; ONE ``MCDEngine.reliability_table`` call follows the
    walk.  Not under a sharded walk (more than one rank): NotImplementedError.

    ``table``: the device tensors of ``reliability_table``; ``metrics``: ``table_metrics`` of it; ``rows``: one ``(name, acc, ece, mce, nll,
    brier)`` per exit and per exit ensemble, named like ``FullAnalysis.all_experiments``' rows; ``labels`` int64 [N]; ``n``.

    ``kde=True``: one more device call after the table, ``MCDEngine.reliability_kde`` on ``grid_points`` grid points — the reference's own
    ``ECE`` column (the KDE-ECE of ``train.metrics.ece_kde_binary``, exact densities).  ``kde``: its device tensors (False without it);
    ``metrics["ece_kde"]`` float64 [R], NaN in a degenerate row (no hit, one hit, equal hit confidences: the reference's NaN); ``rows`` gains
    the value as a seventh element and ``save`` an ``ECE_KDE`` column.

    ``classwise=True``: the walk also fills the classwise records per batch (``MCDEngine.classwise_records``: 4 R C bytes per image) and ONE
    ``MCDEngine.classwise_table`` call (``classwise_bins`` bins, ``classwise_binning`` "width" or "mass") follows it.  ``classwise``: its
    device tensors (False without it); ``metrics`` gains ``cw_ece`` [R] and ``cw_ece_per_class`` [R, C] (``classwise_metrics``); ``rows``
    gains the classwise ECE as one more element, after the KDE value when both are asked for, and ``save`` a ``CW_ECE`` column.  Without
    it nothing of this is allocated or launched."""

    def __init__(self, model, loader, gpu=0, mc_passes=10, seed=0, n_bins=15, binning="mass", kde=False, grid_points=2 ** 14,
                 classwise=False, classwise_bins=15, classwise_binning="width"):
        self.model = model
        self.loader = loader
        self.device = get_device(gpu)
        self.mc_passes = int(mc_passes)
        self.seed = seed
        self.n_bins = int(n_bins)
        self.binning = binning
        self.kde = bool(kde)
        self.grid_points = int(grid_points)
        self.classwise = bool(classwise)
        self.classwise_bins = int(classwise_bins)
        self.classwise_binning = classwise_binning
        if self.classwise and classwise_binning not in ("width", "mass"):
            raise ValueError(f"classwise_binning must be 'width' or 'mass', got {classwise_binning!r}")
        self._run()

    def _engine(self, b_x):
        dtype = self.model.resolve_engine_dtype(self.device, None, calib=b_x, samples=self.mc_passes)
        want = max(b_x.shape[0], int(getattr(self.loader, "batch_size", 0) or 0))
        return self.model.engine(self.device, max_batch=want, dtype=dtype)

    def _capacity(self):
        """The images the loader announces (``FullAnalysis._collect``'s rule): the records' capacity"""
        loader = self.loader
        if getattr(loader, "sampler", None) is not None and hasattr(loader.sampler, "__len__"):
            return len(loader.sampler)
        if hasattr(loader, "dataset"):
            return len(loader.dataset)
        return sum(len(b[1]) for b in loader)

    def _run(self):
        import torch
        from ..sharding import _rank_world
        if _rank_world(None)[1] > 1:
            raise NotImplementedError("ReliabilityAnalysis under a sharded walk: the records are not part of "
                                      "sharding.accumulate_partitioned's all-reduce")
        eng, records, cw_records, labels, off = None, None, None, [], 0
        for k, batch in enumerate(self.loader):
            b_x = batch[0].to(self.device)
            if eng is None:
                eng = self._engine(b_x)
                records = eng.new_reliability_records(max(1, self._capacity()))
                if self.classwise:
                    cw_records = eng.new_classwise_records(max(1, self._capacity()))
            ml = self.model.mask_layers()
            T, seed, cnt0 = self.mc_passes, self.seed + k, (ml[0].cnt if ml else 0)
            self.model.advance(T)
            mean = eng.predict(b_x, T, seed, cnt0=cnt0)["mean"]
            y = torch.as_tensor(np.asarray(batch[1]).astype(np.int64))
            if self.classwise:
                eng.classwise_records(mean, y, cw_records, off)
            off = eng.reliability_records(mean, y, records, off)
            labels.append(y.numpy())
        if eng is None:
            raise ValueError("empty loader")
        self.n = off
        self.labels = np.concatenate(labels)
        self.records = records
        self.table = eng.reliability_table(records, off, self.n_bins, self.binning)
        eng.check_finite()
        self.metrics = table_metrics(self.table, off)
        m = self.metrics
        self.rows = [(name, float(m["acc"][r]), float(m["ece"][r]), float(m["mce"][r]), float(m["nll"][r]), float(m["brier"][r]))
                     for r, name in enumerate(row_names(eng.n_exits))]
        if self.kde:
            self.kde = eng.reliability_kde(records, off, self.grid_points, check=False)
            m["ece_kde"] = np.where(_np(self.kde["degenerate"]) != 0, np.nan, _np(self.kde["ece_kde"]))
            self.rows = [row + (float(v),) for row, v in zip(self.rows, m["ece_kde"])]
        if self.classwise:
            self.classwise_records = cw_records
            self.classwise = eng.classwise_table(cw_records, off, self.classwise_bins, self.classwise_binning, check=False)
            cw = classwise_metrics(self.classwise)
            m["cw_ece"], m["cw_ece_per_class"] = cw["cw_ece"], cw["cw_ece_per_class"]
            self.rows = [row + (float(v),) for row, v in zip(self.rows, m["cw_ece"])]

    def save(self, experiment_id):
        """``test_reliability_<experiment_id>.csv``: a header line, then ``rows``; returns the file name."""
        name = f"test_reliability_{experiment_id}.csv"
        with open(name, "w") as f:
            f.write("Layer,Accuracy,ECE,MCE,NLL,Brier" + (",ECE_KDE" if self.kde else "") + (",CW_ECE" if self.classwise else "") + "\n")
            for r in self.rows:
                f.write(",".join(str(v) for v in r) + "\n")
        return name
