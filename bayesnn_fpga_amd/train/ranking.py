"""Rank quality of the per-image uncertainty scores over a loader: do the wrong predictions — or out-of-distribution inputs — carry the high
uncertainty?  Per exit and per exit ensemble and per score the AUROC of the score as a detector of misclassified (or noise) images and the
risk-coverage curve of selective prediction (keep the most certain fraction c of the images: what error rate do they have?) with its area,
the AURC, and the excess E-AURC over the optimal ranking — formed on the device from exact integers (csrc/ranking.hip:
``MCDEngine.score_records`` per batch and score, ONE ``MCDEngine.rank_quality`` per score at the end).  The reference's hardware evaluation
prints the mean predictive entropy of random-noise inputs (Hardware_Artifact/bayes_hw/data_utils.py:72-90, metric_utils.py:3-6); read per
image, the same data gives these measures.

``score_keys_numpy`` and ``rank_quality_numpy`` restate the device's arithmetic contract (the header comment of csrc/ranking.hip) on the
host; ``rank_metrics``, ``risk_at_coverage`` and ``threshold_at_coverage`` read a table, the device's or the restatement's.
"""
import math

import numpy as np

from .reliability import _np, row_names
from .results_analyzer import get_device

INVALID = 0xFFFFFFFF          # the key of an image that is in no count
MAX_KEY = 0x7F7FFFFF          # the bit pattern of the largest finite float32
SCORES = {"confidence": -1, "pred_entropy": 1, "mutual_info": 1, "variation_ratio": 1, "vote_entropy": 1}     # score -> direction


def _u32(a):
    a = np.ascontiguousarray(_np(a))
    return a.view(np.uint32) if a.dtype == np.int32 else a


def score_keys_numpy(score, direction, valid_keys=None):
    """The host restatement of bmi_score_record: ``score`` [R, B] (float64) -> (ukeys uint32 [R, B], the number of NaN / infinite / negative
    scores).  f = float32(score), round to nearest; where ``valid_keys`` [R, B] is 0 the key is INVALID and nothing is counted; a bad f gives
    INVALID and counts; otherwise b = the bits of f + 0.0 and the key is b (``direction=+1``) or 0x7F7FFFFF - b (``direction=-1``)."""
    if direction not in (1, -1):
        raise ValueError(f"direction must be +1 or -1, got {direction}")
    score = np.asarray(score, dtype=np.float64)
    if score.ndim != 2:
        raise ValueError("score must be [R, B]")
    R, B = score.shape
    silenced = np.zeros((R, B), dtype=bool) if valid_keys is None else _u32(valid_keys) == 0
    if silenced.shape != (R, B):
        raise ValueError("valid_keys must be [R, B]")
    ukeys = np.full((R, B), INVALID, dtype=np.uint32)
    bad = 0
    for r in range(R):
        for n in range(B):                                   # (a float is formed: an explicit loop)
            if silenced[r, n]:
                continue
            with np.errstate(over="ignore", invalid="ignore"):
                f = np.float32(score[r, n])
            if not np.isfinite(f) or f < 0:
                bad += 1
                continue
            b = int((f + np.float32(0.0)).view(np.uint32))
            ukeys[r, n] = b if direction > 0 else MAX_KEY - b
    return ukeys, bad


def rank_quality_numpy(ukeys, positive, n):
    """The host restatement of bmi_rank_quality on columns ``0 .. n - 1`` of ``ukeys`` (uint32 or int32 [R, capacity]) and ``positive``
    ([R, capacity], non-zero: positive): dict(rank int32 [R, n], sorted_keys uint32 [R, n], curve int32 [R, n], counts int64 [R, 3] =
    (m, n_pos, U2), aurc_sum float64 [R], n).  The order is ``np.argsort(kind="stable")`` of the valid keys (a key above 0x7F7FFFFF is
    invalid), the curve a ``cumsum``; U2 comes from the positives before each negative and the tie groups; ``aurc_sum`` is an explicit
    ascending loop of float64 divisions."""
    ukeys, positive, n = _u32(ukeys), np.asarray(_np(positive)), int(n)
    if ukeys.dtype != np.uint32 or ukeys.ndim != 2 or positive.shape != ukeys.shape or not 1 <= n <= ukeys.shape[1]:
        raise ValueError("ukeys uint32 / int32 [R, capacity], positive [R, capacity], 1 <= n <= capacity")
    R = ukeys.shape[0]
    out = dict(rank=np.full((R, n), -1, dtype=np.int32), sorted_keys=np.full((R, n), INVALID, dtype=np.uint32),
               curve=np.zeros((R, n), dtype=np.int32), counts=np.zeros((R, 3), dtype=np.int64), aurc_sum=np.zeros(R, dtype=np.float64), n=n)
    for r in range(R):
        u = ukeys[r, :n]
        at = np.nonzero(u <= MAX_KEY)[0]                     # the valid images, in image order
        m = len(at)
        order = at[np.argsort(u[at], kind="stable")]
        pos = (positive[r, :n] != 0)[order].astype(np.int64)
        su = u[order]
        cum = np.cumsum(pos)
        n_pos = int(cum[-1]) if m else 0
        out["rank"][r, order] = np.arange(m, dtype=np.int32)
        out["sorted_keys"][r, :m] = su
        out["curve"][r, :m] = cum
        out["curve"][r, m:] = n_pos
        # per positive image: the negatives with a smaller key count 2, with an equal key 1
        neg_cum = np.cumsum(1 - pos)
        first = np.searchsorted(su, su, side="left")         # the first position of each image's tie group, and one past its last
        last = np.searchsorted(su, su, side="right")
        neg_before = np.where(first > 0, neg_cum[np.maximum(first - 1, 0)], 0) if m else neg_cum
        neg_upto = neg_cum[last - 1] if m else neg_cum
        u2 = int((pos * (2 * neg_before + (neg_upto - neg_before))).sum()) if m else 0
        out["counts"][r] = (m, n_pos, u2)
        s = 0.0
        for k, c in enumerate(cum.tolist()):                 # position order
            s = s + float(c) / float(k + 1)
        out["aurc_sum"][r] = s
    return out


def rank_metrics(table):
    """float64 on the host, from a table of ``MCDEngine.rank_quality`` or ``rank_quality_numpy``: dict(auroc, aurc, eaurc, m, n_pos), each
    [R].  auroc = U2 / (2 n_pos n_neg), NaN where n_pos or n_neg is 0; aurc = aurc_sum / m, NaN where m is 0; eaurc = aurc minus the
    area of the optimal ranking — every negative before every positive —, sum_{j=1..n_pos} j / (m - n_pos + j) / m, added in ascending j
    (the loop of ``aurc_sum`` on that ranking, whose first m - n_pos terms are 0)."""
    counts = _np(table["counts"]).astype(np.int64)
    aurc_sum = _np(table["aurc_sum"]).astype(np.float64)
    R = counts.shape[0]
    out = dict(auroc=np.full(R, np.nan), aurc=np.full(R, np.nan), eaurc=np.full(R, np.nan), m=counts[:, 0].copy(), n_pos=counts[:, 1].copy())
    for r in range(R):
        m, n_pos, u2 = (int(v) for v in counts[r])
        n_neg = m - n_pos
        if n_pos and n_neg:
            out["auroc"][r] = float(u2) / float(2 * n_pos * n_neg)
        if m:
            best = 0.0
            for j in range(1, n_pos + 1):
                best = best + float(j) / float(n_neg + j)
            out["aurc"][r] = aurc_sum[r] / float(m)
            out["eaurc"][r] = aurc_sum[r] / float(m) - best / float(m)
    return out


def _position(m, c):
    """k = ceil(c m) clipped to [1, m]: the number of images kept at coverage ``c``"""
    return min(max(int(math.ceil(float(c) * m)), 1), m)


def risk_at_coverage(table, c):
    """The selective risk at coverage ``c``, float64 [R]: curve[k - 1] / k with k = ceil(c m) clipped to [1, m] — the share of positive
    (wrong) images among the k most certain ones.  NaN where m is 0."""
    counts, curve = _np(table["counts"]), _np(table["curve"])
    out = np.full(counts.shape[0], np.nan)
    for r in range(counts.shape[0]):
        m = int(counts[r, 0])
        if m:
            k = _position(m, c)
            out[r] = float(curve[r, k - 1]) / float(k)
    return out


def threshold_at_coverage(table, c, direction):
    """The score of the least certain image kept at coverage ``c``, float32 [R], decoded from sorted_keys[k - 1] (k as in
    ``risk_at_coverage``; ``direction``: the one the keys were recorded with): accepting the images whose score is at most this value
    (``direction=+1``; at least this value for a confidence, ``direction=-1``) keeps at least k of them, with the risk
    ``risk_at_coverage`` reports when the value is not tied across position k — the threshold to hand to ``predict_early_exit`` or
    ``predict_adaptive``.  NaN where m is 0."""
    if direction not in (1, -1):
        raise ValueError(f"direction must be +1 or -1, got {direction}")
    counts, keys = _np(table["counts"]), _u32(table["sorted_keys"])
    out = np.full(counts.shape[0], np.nan, dtype=np.float32)
    for r in range(counts.shape[0]):
        m = int(counts[r, 0])
        if m:
            key = int(keys[r, _position(m, c) - 1])
            out[r] = np.uint32(key if direction > 0 else MAX_KEY - key).view(np.float32)
    return out


def _images(batch):
    return batch[0] if isinstance(batch, (tuple, list)) else batch


class RankingAnalysis:
    """One walk of ``loader`` (batches ``(x, y, ...)``) with ``mc_passes`` stochastic passes per batch, the rank quality of ``scores``
    formed on the device.  The walk is ``ReliabilityAnalysis``'s: batch k runs under seed ``seed + k`` with the model's current Masksembles
    counter, the counters advance by ``mc_passes`` afterwards (``model.advance``), the engine is the model's.  Per batch:
    ``MCDEngine.predict_votes``, ``reliability_records`` (the hit bits and the confidence keys), one ``score_records`` call per score; ONE
    ``rank_quality`` call per score follows the walk.  Not under a sharded walk (more than one rank): NotImplementedError.

    Rows are ``row_names``': the exits, then the exit ensembles (the ``ens_*`` entries of ``predict_votes``).  Scores: "confidence" (the
    float32 confidence of the T-mean prediction in the reliability records' ``keys``, direction -1), "pred_entropy", "mutual_info",
    "variation_ratio", "vote_entropy" (direction +1).  ``positive = 1 - hit`` where ``hit`` is THE T-MEAN PREDICTION'S for every score,
    the vote scores included: the question is whether the score flags the errors of the prediction a caller reads.  An image with a bad
    label or a non-finite row is in no count (``valid``: the reliability keys).

    ``tables``: score -> the device tensors of ``rank_quality``; ``metrics``: score -> ``rank_metrics`` plus ``risk80`` (the risk at 0.8
    coverage); ``rows``: one ``(name, score, auroc, aurc, eaurc, risk80)`` per row and score; ``labels`` int64 [N]; ``n``.

    ``ood_loader``: batches of out-of-distribution images (``bayesnn_fpga_amd.synthetic.synthetic_images`` gives noise; labels, if any,
    are ignored).  The walk goes on over them (seeds ``seed + k`` continue), their scores go into the columns behind the ``n``
    in-distribution ones, ``positive`` is 1 there and 0 in front, validity is by finiteness only, and a second ``rank_quality`` per score
    gives ``ood_tables`` / ``ood_metrics``; ``ood_rows``: one ``(name, score, auroc, ape_in, ape_noise)`` per row and score; ``ape``: the mean
    predictive entropy per row, (in-distribution float64 [R], noise float64 [R]) — the pair the reference prints; ``n_ood``."""

    def __init__(self, model, loader, gpu=0, mc_passes=10, seed=0, scores=("confidence", "pred_entropy", "mutual_info", "variation_ratio"),
                 ood_loader=None):
        self.model = model
        self.loader = loader
        self.ood_loader = ood_loader
        self.device = get_device(gpu)
        self.mc_passes = int(mc_passes)
        self.seed = seed
        self.scores = tuple(scores)
        unknown = [s for s in self.scores if s not in SCORES]
        if unknown or not self.scores:
            raise ValueError(f"scores must be among {sorted(SCORES)}, got {unknown or self.scores}")
        self._run()

    def _engine(self, b_x):
        dtype = self.model.resolve_engine_dtype(self.device, None, calib=b_x, samples=self.mc_passes)
        want = max(b_x.shape[0], int(getattr(self.loader, "batch_size", 0) or 0), int(getattr(self.ood_loader, "batch_size", 0) or 0))
        return self.model.engine(self.device, max_batch=want, dtype=dtype)

    @staticmethod
    def _capacity(loader):
        if loader is None:
            return 0
        if getattr(loader, "sampler", None) is not None and hasattr(loader.sampler, "__len__"):
            return len(loader.sampler)
        if hasattr(loader, "dataset"):
            return len(loader.dataset)
        return sum(len(_images(b)) for b in loader)

    def _run(self):
        import torch
        from ..sharding import _rank_world
        if _rank_world(None)[1] > 1:
            raise NotImplementedError("RankingAnalysis under a sharded walk: the score records are not part of "
                                      "sharding.accumulate_partitioned's all-reduce")
        n_in, n_out = self._capacity(self.loader), self._capacity(self.ood_loader)
        if n_in < 1:
            raise ValueError("empty loader")
        eng, rel, rec, ood_rec, labels, off, k = None, None, {}, {}, [], 0, 0
        ape_sum = None
        for ood, loader in ((False, self.loader), (True, self.ood_loader)):
            if loader is None:
                continue
            for batch in loader:
                b_x = _images(batch).to(self.device)
                B = b_x.shape[0]
                if eng is None:
                    eng = self._engine(b_x)
                    R = 2 * eng.n_exits
                    rel = eng.new_reliability_records(n_in + n_out)
                    rec = {s: eng.new_score_records(n_in + n_out, R) for s in self.scores}
                    ood_rec = {s: eng.new_score_records(n_in + n_out, R) for s in self.scores} if n_out else {}
                    ape_sum = torch.zeros(2, R, dtype=torch.float64, device=self.device)
                ml = self.model.mask_layers()
                T, seed, cnt0 = self.mc_passes, self.seed + k, (ml[0].cnt if ml else 0)
                self.model.advance(T)
                r = eng.predict_votes(b_x, T, seed, cnt0=cnt0)
                # (a noise image has no label: the record of label 0 holds the same confidence, and its hit bit is not read)
                y = torch.zeros(B, dtype=torch.int64) if ood else torch.as_tensor(np.asarray(batch[1]).astype(np.int64))
                eng.reliability_records(r["mean"], y, rel, off)
                if not ood:
                    labels.append(y.numpy())
                ape_sum[int(ood)] += torch.cat([r["pred_entropy"], r["ens_pred_entropy"]]).sum(dim=1)
                for s in self.scores:
                    if s == "confidence":
                        score = rel["keys"][:, off:off + B].contiguous().view(torch.float32).to(torch.float64)
                    else:
                        score = torch.cat([r[s], r["ens_" + s]]).contiguous()
                    if not ood:
                        eng.score_records(score, rec[s], off, SCORES[s], valid=rel["keys"])
                    if n_out:                                # validity by finiteness only
                        eng.score_records(score, ood_rec[s], off, SCORES[s])
                off += B
                k += 1
            if not ood:
                self.n = off
        self.n_ood = off - self.n
        self.labels = np.concatenate(labels)
        self.records = rel
        positive = 1 - rel["hit"]
        self.tables = {s: eng.rank_quality(rec[s]["ukeys"], positive, self.n) for s in self.scores}
        eng.check_finite()
        self.metrics, self.rows = {}, []
        names = row_names(eng.n_exits)
        for s in self.scores:
            m = self.metrics[s] = rank_metrics(self.tables[s])
            m["risk80"] = risk_at_coverage(self.tables[s], 0.8)
        for r, name in enumerate(names):
            for s in self.scores:
                m = self.metrics[s]
                self.rows.append((name, s, float(m["auroc"][r]), float(m["aurc"][r]), float(m["eaurc"][r]), float(m["risk80"][r])))
        self.ood_tables, self.ood_metrics, self.ood_rows, self.ape = {}, {}, [], None
        if self.n_ood:
            total = self.n + self.n_ood
            positive = torch.zeros(2 * eng.n_exits, n_in + n_out, dtype=torch.uint8, device=self.device)
            positive[:, self.n:total] = 1
            for s in self.scores:
                self.ood_tables[s] = eng.rank_quality(ood_rec[s]["ukeys"], positive, total)
                self.ood_metrics[s] = rank_metrics(self.ood_tables[s])
            ape = _np(ape_sum)
            self.ape = (ape[0] / float(self.n), ape[1] / float(self.n_ood))
            self.ood_rows = [(name, s, float(self.ood_metrics[s]["auroc"][r]), float(self.ape[0][r]), float(self.ape[1][r]))
                             for r, name in enumerate(names) for s in self.scores]

    def save(self, experiment_id):
        """``test_ranking_<experiment_id>.csv``: a header line, then ``rows`` (with the out-of-distribution AUROC as a last column under
        ``ood_loader``); returns the file name."""
        name = f"test_ranking_{experiment_id}.csv"
        ood = {(r[0], r[1]): r[2] for r in self.ood_rows}
        with open(name, "w") as f:
            f.write("Layer,Score,AUROC,AURC,E-AURC,Risk@0.8" + (",AUROC_OOD" if ood else "") + "\n")
            for r in self.rows:
                f.write(",".join(str(v) for v in r + ((ood[r[:2]],) if ood else ())) + "\n")
        return name
