"""Exit-policy sweep over a loader: for every confidence threshold, what accuracy, calibration and cost the network reaches when each image
leaves at the first confident exit — the trade-off table of ``FullAnalysis.get_confidence_exiting_values`` (SA/train/results_analyzer.py:
543-566: ``confidence_exiting`` :606-630, ``flop_saver`` :638-670, ``flop_saver_ensembled`` :672-723) formed on the device from per-image
records (csrc/exit_policy.hip: ``MCDEngine.exit_stat_records`` per batch beside ``reliability_records``, ``MCDEngine.exit_policy_sweep`` after
the walk), decided in the arithmetic of ``predict_early_exit``'s own rule and costed with what the staged engine runs.

``exit_stat_numpy`` and ``exit_policy_numpy`` restate the two device calls loop by loop; ``reference_costs`` are the reference's per-exit
FLOP vectors, ``stage_costs`` / ``policy_macs`` the staged engine's cost model; ``policy_metrics`` derives accuracy, exit histogram and cost
from a sweep, the device's or the restatement's.
"""
import struct

import numpy as np

from .confidence_exiting import CONFIDENCE_LIST, FLOPS, baseline_flops
from .reliability import ReliabilityAnalysis, _np, table_metrics
from .results_analyzer import get_device

RULES = ("confidence", "margin")
MAX_THRESHOLDS, MAX_RECORD_ROWS = 1024, 64      # BMI_POLICY_MAX_* of bmi_exit_policy_sweep


def exit_stat_numpy(S1, t_count, rule="confidence", weights=None):
    """The host restatement of bmi_exit_stat_record — of ``exit_rule_stat`` in csrc/exit_rule.h: ``S1`` float64 [E, B, C] (the sums of
    ``t_count`` samples' probabilities), ``weights`` float64 [E, E] or None.  Returns float64 [2, E, B]: plane 0 the exits' own statistic,
    plane 1 the exit ensembles' (row e of ``weights`` over exits 0..e, or their equal mean).  p_c = S1 / t — a division, not a product
    with 1 / t —; the ensemble's exits are added in exit order; the two largest p_c are found by the rule's own ascending loop over the
    classes (a NaN p_c fails both comparisons and is passed over); confidence = top-1, margin = top-1 minus top-2 (top-1 alone when
    C = 1).  No step is fused."""
    S1 = np.asarray(S1, dtype=np.float64)
    if S1.ndim != 3:
        raise ValueError("S1 must be [E, B, C]")
    if rule not in RULES:
        raise ValueError(f"rule must be one of {RULES}, got {rule!r}")
    E, B, Cd = S1.shape
    t = float(int(t_count))
    W = None if weights is None else np.asarray(weights, dtype=np.float64).reshape(E, E)
    out = np.empty((2, E, B), dtype=np.float64)
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        for ens in range(2):
            for e in range(E):
                m1 = np.full(B, -1.0)
                m2 = np.full(B, -1.0)
                for c in range(Cd):
                    if ens and W is not None:
                        p = np.zeros(B)
                        for x in range(e + 1):
                            p = p + W[e, x] * (S1[x, :, c] / t)
                    elif ens:
                        acc = np.zeros(B)
                        for x in range(e + 1):
                            acc = acc + S1[x, :, c] / t
                        p = acc / float(e + 1)
                    else:
                        p = S1[e, :, c] / t
                    first = p > m1
                    second = ~first & (p > m2)
                    m2 = np.where(first, m1, np.where(second, p, m2))
                    m1 = np.where(first, p, m1)
                out[ens, e] = m1 - (m2 if Cd > 1 else 0.0) if rule == "margin" else m1
    return out


def exit_policy_numpy(stat, thresholds, keys, hit, nll, brier, n=None, first_exit=1, select=False):
    """The host restatement of bmi_exit_policy_sweep: ``stat`` float64 [E, capacity] (one plane of the statistic record), ``thresholds``
    float64 [G], the outcome rows ``keys`` (uint32 or int32), ``hit``, ``nll``, ``brier`` [E, capacity], columns ``0 .. n - 1``.  Per threshold
    and image, an explicit walk: e* = the lowest e in [first_exit, E-2] with stat[e][n] > threshold (strict; false for a NaN), else E-1; an
    image whose outcome key at e* is 0 counts in ``invalid`` only.  Returns dict(count, hits int64 [G, E], invalid int64 [G], exit_of uint8
    [G, capacity], n) and with ``select`` also ``selected``: dict(keys uint32, hit uint8, nll, brier float64 [G, capacity]) — the four records
    at (e*, n), zeros for an invalid image and beyond ``n``."""
    stat = np.asarray(_np(stat), dtype=np.float64)
    keys = np.ascontiguousarray(_np(keys))
    if keys.dtype == np.int32:
        keys = keys.view(np.uint32)
    hit, nll, brier = np.asarray(_np(hit)), np.asarray(_np(nll), dtype=np.float64), np.asarray(_np(brier), dtype=np.float64)
    thr = np.asarray(_np(thresholds), dtype=np.float64).reshape(-1)
    E, cap = stat.shape
    n, G, first_exit = int(cap if n is None else n), thr.shape[0], int(first_exit)
    if not (keys.shape == hit.shape == nll.shape == brier.shape == (E, cap)) or not 1 <= n <= cap:
        raise ValueError("stat and the four outcome rows are [E, capacity], 1 <= n <= capacity")
    if not 0 <= first_exit < E or G < 1:
        raise ValueError("first_exit in [0, E), at least one threshold")
    count = np.zeros((G, E), dtype=np.int64)
    hits = np.zeros((G, E), dtype=np.int64)
    invalid = np.zeros(G, dtype=np.int64)
    exit_of = np.zeros((G, cap), dtype=np.uint8)
    sel = dict(keys=np.zeros((G, cap), dtype=np.uint32), hit=np.zeros((G, cap), dtype=np.uint8), nll=np.zeros((G, cap)), brier=np.zeros((G, cap)))
    cols = np.arange(n)
    with np.errstate(invalid="ignore"):
        for g in range(G):
            taken = np.full(n, E - 1, dtype=np.int64)
            for e in range(E - 2, first_exit - 1, -1):           # descending, so that the lowest confident exit is written last
                taken = np.where(stat[e, :n] > thr[g], e, taken)
            exit_of[g, :n] = taken
            ok = keys[taken, cols] != 0
            invalid[g] = int((~ok).sum())
            for e in range(E):
                at = ok & (taken == e)
                count[g, e] = int(at.sum())
                hits[g, e] = int((hit[e, :n][at] != 0).sum())
            if select:
                sel["keys"][g, :n] = np.where(ok, keys[taken, cols], 0)
                sel["hit"][g, :n] = np.where(ok, hit[taken, cols], 0)
                sel["nll"][g, :n] = np.where(ok, nll[taken, cols], 0.0)
                sel["brier"][g, :n] = np.where(ok, brier[taken, cols], 0.0)
    out = dict(count=count, hits=hits, invalid=invalid, exit_of=exit_of, thresholds=thr, n=n)
    if select:
        out["selected"] = sel
    return out


def reference_costs(model_type, exit_only, mc_passes=10, ensembled=False):
    """int64 [E]: what the reference charges an image that leaves at exit e — the ``cost`` vector of ``flop_saver`` (``ensembled``: of
    ``flop_saver_ensembled``), from ``confidence_exiting.FLOPS`` (fvcore counts the reference hard-codes)."""
    f = FLOPS[model_type]
    per_layer = np.cumsum(np.array(f["layer"], dtype=np.int64))
    convs, fc = np.array(f["exit_convs"], dtype=np.int64), np.array(f["exit_fc"], dtype=np.int64)
    if ensembled:
        convs, fc = np.cumsum(convs), np.cumsum(fc)
    if exit_only:
        return per_layer + convs + int(mc_passes) * fc
    return int(mc_passes) * (per_layer + convs + fc)


def stage_costs(stages, T, first_exit, n_exits):
    """The cost model of the staged engine from its stage plan (``CompiledGraph.exit_stages(first_exit)``: one dict per stage with
    prefix_macs, suffix_macs, whole_batch_macs) at ``T`` samples: dict(per_exit — E Python ints, the cumulative MACs of the stages an image
    that leaves at exit e ran, each stage's prefix MACs without its whole-batch ops plus T x its suffix MACs; 0 before ``first_exit`` —,
    stage_macs, whole_batch_macs (per stage and image; run over the WHOLE batch whenever anybody reaches the stage), T, first_exit)."""
    T, first_exit, n_exits = int(T), int(first_exit), int(n_exits)
    if T < 1 or not 0 <= first_exit < n_exits or len(stages) != n_exits - first_exit:
        raise ValueError("T >= 1, first_exit in [0, E) and one stage per exit from first_exit on")
    stage = [int(st["prefix_macs"]) - int(st["whole_batch_macs"]) + T * int(st["suffix_macs"]) for st in stages]
    per_exit, run = [0] * n_exits, 0
    for k, c in enumerate(stage):
        run += c
        per_exit[first_exit + k] = run
    return dict(per_exit=per_exit, stage_macs=stage, whole_batch_macs=[int(st["whole_batch_macs"]) for st in stages], T=T, first_exit=first_exit)


def policy_macs(count_row, costs, B):
    """The MACs ``predict_early_exit`` runs on a batch of ``B`` images of which ``count_row[e]`` leave at exit e (``costs``:
    ``MCDEngine.exit_costs`` / ``stage_costs``) — its ``macs_done``, as a Python int: stage k is run by the images that leave at exit
    first_exit + k or later, its whole-batch ops by all ``B``, and a stage nobody reaches adds nothing.  The row must account for every
    image (an invalid image is in no count, and what it ran is not known from the counts): ValueError otherwise."""
    row = [int(v) for v in _np(count_row).reshape(-1)]
    B, fe = int(B), int(costs["first_exit"])
    stage, whole = costs["stage_macs"], costs["whole_batch_macs"]
    if len(row) != fe + len(stage) or any(v < 0 for v in row):
        raise ValueError("count_row holds one non-negative count per exit")
    if sum(row) != B or any(row[:fe]):
        raise ValueError(f"the counts cover {sum(row)} of {B} images, {sum(row[:fe])} of them before first_exit")
    done = 0
    for k in range(len(stage)):
        ran = sum(row[fe + k:])
        if ran == 0:
            break
        done += ran * stage[k] + B * whole[k]
    return done


def policy_metrics(sweep, costs, n=None):
    """From a sweep (``MCDEngine.exit_policy_sweep`` or ``exit_policy_numpy``): dict(accuracy float64 [G] = sum_e hits / n, exit_hist int64
    [G, E] = the count rows, invalid int64 [G], cost: a list of G exact Python ints).  ``costs``: a per-exit vector (``reference_costs``:
    cost = sum_e count[g][e] * costs[e]) or the dict of ``MCDEngine.exit_costs`` (cost = ``policy_macs(count[g], costs, n)``: the whole
    set costed as one batch)."""
    n = int(sweep["n"] if n is None else n)
    count, hits = _np(sweep["count"]).astype(np.int64), _np(sweep["hits"]).astype(np.int64)
    if isinstance(costs, dict):
        cost = [policy_macs(row, costs, n) for row in count]
    else:
        per = [int(v) for v in np.asarray(costs).reshape(-1)]
        if len(per) != count.shape[1]:
            raise ValueError("one cost per exit")
        cost = [sum(int(c) * p for c, p in zip(row, per)) for row in count]
    return dict(accuracy=hits.sum(axis=1) / float(n), exit_hist=count, invalid=_np(sweep["invalid"]).astype(np.int64), cost=cost)


def _ordinal(x):
    """float64 -> a Python int whose order is the float order (-0.0 and +0.0 both 0); _from_ordinal inverts it"""
    b = struct.unpack("<q", struct.pack("<d", float(x)))[0]
    return b if b >= 0 else -(b & 0x7FFFFFFFFFFFFFFF)


def _from_ordinal(o):
    return struct.unpack("<d", struct.pack("<Q", o if o >= 0 else (-o) | (1 << 63)))[0]


class ExitPolicyAnalysis:
    """One walk of ``loader`` (batches ``(x, y, ...)``) with ``mc_passes`` stochastic passes per batch, then the exit policy of every
    threshold on the device.  The walk is ``ReliabilityAnalysis``'s: batch k runs under seed ``seed + k`` with the model's current
    Masksembles counter, the counters advance by ``mc_passes`` afterwards (``model.advance``), the engine is the model's
    (``engine_dtype="auto"`` applies).  Per batch the moment sums are kept (``accumulate`` + ``finalize``) and two records written:
    ``reliability_records`` (the outcome at every exit and exit ensemble) and ``exit_stat_records`` (the decision statistic of ``rule`` in
    ``predict_early_exit``'s arithmetic).  After the walk ``exit_policy_sweep`` runs twice — the per-exit policy and the exit-ensemble
    policy — with the selected records, which go to ``reliability_table`` (``n_bins`` equal-mass bins) and, with ``kde``, to
    ``reliability_kde``.  At most 64 thresholds (the rows a table takes).

    ``rows``: one dict per threshold, in the order given — threshold, and for the per-exit policy accuracy, ece, nll, brier, exits (the
    images leaving at each exit), flops / flops_rel (the reference's FLOPs by ``reference_costs``, and relative to ``baseline_flops`` x n:
    what the reference prints; None for a model family the reference has no counts for) and macs / macs_rel (the staged engine's own MACs
    by ``policy_macs`` with the whole set costed as one batch, and relative to ``predict``'s), with ``kde`` also ece_kde (NaN in a
    degenerate row); the same under ``ens_`` for the ensemble policy.  ``sweeps`` / ``tables`` / ``kdes``: the device tensors of both
    policies, index 0 per exit, 1 ensemble.  ``save`` writes the CSV; ``threshold_for_budget`` inverts the cost.

    Not under a sharded walk (more than one rank), and not while ensemble weights are set — the ensemble policy's outcome rows are the
    equal-mean ensemble's —: NotImplementedError."""

    def __init__(self, model, loader, gpu=0, mc_passes=10, seed=0, thresholds=CONFIDENCE_LIST, rule="confidence", first_exit=1, n_bins=15,
                 kde=False, grid_points=2 ** 14):
        self.model = model
        self.loader = loader
        self.device = get_device(gpu)
        self.mc_passes = int(mc_passes)
        self.seed = seed
        self.thresholds = [float(t) for t in thresholds]
        self.rule = rule
        self.first_exit = int(first_exit)
        self.n_bins = int(n_bins)
        self.kde = bool(kde)
        self.grid_points = int(grid_points)
        if rule not in RULES:
            raise ValueError(f"rule must be one of {RULES}, got {rule!r}")
        if not 1 <= len(self.thresholds) <= MAX_RECORD_ROWS:
            raise ValueError(f"ExitPolicyAnalysis takes 1 .. {MAX_RECORD_ROWS} thresholds")
        self._run()

    _engine = ReliabilityAnalysis._engine            # the model's engine at the loader's batch size, the records' capacity: its rules
    _capacity = ReliabilityAnalysis._capacity

    def _reference(self):
        """(model_type, exit_only) as FullAnalysis reads them off the model, or (None, None)"""
        fam = getattr(self.model, "family", None)
        model_type = {"vgg": "vgg19", "resnet": "resnet18"}.get(fam)
        if model_type is None or len(FLOPS[model_type]["layer"]) != self.eng.n_exits:
            return None, None
        dropout = getattr(self.model, "dropout", None)
        return model_type, bool(getattr(self.model, "dropout_exit", True) and dropout is None)

    def _run(self):
        import torch
        from ..sharding import _rank_world
        if _rank_world(None)[1] > 1:
            raise NotImplementedError("ExitPolicyAnalysis under a sharded walk: the records are not part of "
                                      "sharding.accumulate_partitioned's all-reduce")
        eng, rel, stat, labels, off = None, None, None, [], 0
        T = self.mc_passes
        for k, batch in enumerate(self.loader):
            b_x = batch[0].to(self.device)
            if eng is None:
                eng = self._engine(b_x)
                if eng.ensemble_weights is not None:
                    raise NotImplementedError("ExitPolicyAnalysis while ensemble weights are set: the reliability records' ensemble rows "
                                              "are the equal-mean ensemble's, not the weighted one the rule would decide on")
                if not 0 <= self.first_exit < eng.n_exits:
                    raise ValueError(f"first_exit must be in [0, {eng.n_exits})")
                cap = max(1, self._capacity())
                rel, stat = eng.new_reliability_records(cap), eng.new_exit_stat_records(cap)
            ml = self.model.mask_layers()
            seed, cnt0 = self.seed + k, (ml[0].cnt if ml else 0)
            self.model.advance(T)
            S = eng.new_moments(b_x.shape[0])
            eng.accumulate(b_x, S, 0, T, seed, cnt0)
            mean = eng.finalize(S, T)["mean"]
            y = torch.as_tensor(np.asarray(batch[1]).astype(np.int64))
            eng.exit_stat_records(S, T, stat, off, self.rule)
            off = eng.reliability_records(mean, y, rel, off)
            labels.append(y.numpy())
        if eng is None:
            raise ValueError("empty loader")
        self.eng, self.n = eng, off
        self.labels = np.concatenate(labels)
        self.records, self.stat_records = rel, stat
        nonfinite, badlabel = (int(v) for v in rel["counters"].tolist())
        if nonfinite:
            raise FloatingPointError(f"{nonfinite} reliability records with a non-finite probability on the {eng.dtype!r} engine")
        if badlabel:
            raise ValueError(f"{badlabel} images with a label outside [0, C) in the reliability records")
        eng.check_finite()
        self.model_type, self.exit_only = self._reference()
        self.costs = eng.exit_costs(T, self.first_exit)
        self.sweeps, self.tables, self.kdes, self.metrics = [], [], [], []
        for ens in (False, True):
            sw = eng.exit_policy_sweep(stat, rel, off, self.thresholds, ensemble=ens, first_exit=self.first_exit, select=True)
            table = eng.reliability_table(sw["selected"], off, self.n_bins, "mass", check=False)
            m = table_metrics(table, off)
            if self.kde:
                kd = eng.reliability_kde(sw["selected"], off, self.grid_points, check=False)
                m["ece_kde"] = np.where(_np(kd["degenerate"]) != 0, np.nan, _np(kd["ece_kde"]))
                self.kdes.append(kd)
            m["macs"] = policy_metrics(sw, self.costs, off)["cost"]
            pm = policy_metrics(sw, self._ref_costs(ens) if self.model_type else [0] * eng.n_exits, off)
            m["flops"] = pm["cost"] if self.model_type else [None] * len(self.thresholds)
            m["accuracy"], m["exits"] = pm["accuracy"], pm["exit_hist"]
            self.sweeps.append(sw)
            self.tables.append(table)
            self.metrics.append(m)
        base = baseline_flops(self.model_type) * off if self.model_type else None
        full = self.costs["macs_full"] * off
        self.rows = []
        for g, th in enumerate(self.thresholds):
            row = dict(threshold=th)
            for m, pre in zip(self.metrics, ("", "ens_")):
                row.update({pre + "accuracy": float(m["accuracy"][g]), pre + "ece": float(m["ece"][g]), pre + "nll": float(m["nll"][g]),
                            pre + "brier": float(m["brier"][g]), pre + "exits": [int(v) for v in m["exits"][g]], pre + "flops": m["flops"][g],
                            pre + "flops_rel": None if base is None else m["flops"][g] / base, pre + "macs": m["macs"][g],
                            pre + "macs_rel": m["macs"][g] / full})
                if self.kde:
                    row[pre + "ece_kde"] = float(m["ece_kde"][g])
            self.rows.append(row)

    def _ref_costs(self, ensemble):
        return reference_costs(self.model_type, self.exit_only, self.mc_passes, ensembled=bool(ensemble))

    def policy_costs(self, thresholds, ensemble=False, engine_cost=True):
        """The cost of each threshold as exact Python ints, from one more sweep of the records on the device (counts only): the engine's
        MACs (``engine_cost``) or the reference's FLOPs"""
        sw = self.eng.exit_policy_sweep(self.stat_records, self.records, self.n, thresholds, ensemble=ensemble, first_exit=self.first_exit)
        if not engine_cost and self.model_type is None:
            raise ValueError("the reference has no FLOP counts for this model family")
        return policy_metrics(sw, self.costs if engine_cost else self._ref_costs(ensemble), self.n)["cost"]

    def threshold_for_budget(self, max_cost, ensemble=False, engine_cost=True):
        """The highest float64 threshold whose policy costs at most ``max_cost`` over the walked images (the engine's MACs with the whole
        set costed as one batch, or with ``engine_cost=False`` the reference's FLOPs).  The cost never falls as the threshold rises, so the
        thresholds that fit are everything below one statistic value: the answer is bracketed on the current grid (and at -inf / +inf
        beyond it), then the sweep runs again on up to 1024 thresholds spread over the float64 values between the two neighbours until
        they are adjacent — at most seven calls, the records never leave the device.  +inf when even the full network fits; ValueError
        when not even leaving everything at ``first_exit`` does."""
        max_cost = int(max_cost)
        grid = sorted(set(self.thresholds) | {float("-inf"), float("inf")})
        cost = self.policy_costs(grid, ensemble, engine_cost)
        if cost[0] > max_cost:
            raise ValueError(f"no threshold fits: leaving every image at exit {self.first_exit} costs {cost[0]} > {max_cost}")
        fits = [c <= max_cost for c in cost]
        if all(fits):
            return float("inf")
        first_over = fits.index(False)                       # (the cost is monotone: everything before it fits)
        lo, hi = _ordinal(grid[first_over - 1]), _ordinal(grid[first_over])
        while hi - lo > 1:
            pts = sorted({lo + (hi - lo) * k // (MAX_THRESHOLDS + 1) for k in range(1, MAX_THRESHOLDS + 1)} - {lo, hi})
            cost = self.policy_costs([_from_ordinal(o) for o in pts], ensemble, engine_cost)
            for o, c in zip(pts, cost):
                if c <= max_cost:
                    lo = o
                else:
                    hi = o
                    break
        return _from_ordinal(lo)

    def save(self, experiment_id):
        """``test_exit_policy_<experiment_id>.csv``: a header line, then per threshold the per-exit policy's row and the ``Ensemble`` row,
        as the reference prints them (threshold, accuracy, ECE, relative FLOPs, NLL), with the Brier score, the engine's relative MACs and the
        exit histogram beside them; returns the file name."""
        name = f"test_exit_policy_{experiment_id}.csv"
        with open(name, "w") as f:
            f.write("Policy,Threshold,Accuracy,ECE,FLOPs_rel,NLL,Brier,MACs_rel,FLOPs,MACs,Exits" + (",ECE_KDE" if self.kde else "") + "\n")
            for r in self.rows:
                for pre, tag in (("", "E"), ("ens_", "Ensemble")):
                    vals = [tag, r["threshold"], r[pre + "accuracy"], r[pre + "ece"], r[pre + "flops_rel"], r[pre + "nll"], r[pre + "brier"],
                            r[pre + "macs_rel"], r[pre + "flops"], r[pre + "macs"], " ".join(str(v) for v in r[pre + "exits"])]
                    if self.kde:
                        vals.append(r[pre + "ece_kde"])
                    f.write(",".join("" if v is None else str(v) for v in vals) + "\n")
        return name

