"""Conformal prediction sets over a loader: split conformal prediction per exit and per exit ensemble — LAC (Sadinle et al. 2019), APS
(Romano et al. 2020, the deterministic form) and RAPS (Angelopoulos et al. 2021) —, formed on the device from the classwise records
(csrc/conformal.hip: ``MCDEngine.conformal_scores`` / ``conformal_quantile`` on a calibration loader, ``MCDEngine.conformal_sets`` on a
test loader) in integer arithmetic.  The calibration map in force (temperature, vector, matrix) is the engine's: RAPS is defined on
calibrated probabilities.

``conformal_numpy`` restates the device's arithmetic contract (the header comment of csrc/conformal.hip) on the host, loop by loop;
``conformal_metrics`` derives the coverage figures from the tables, the device's or the restatement's.
"""
import numpy as np

from .reliability import INVALID, _np
from .results_analyzer import get_device

METHODS = ("lac", "aps", "raps")
UNIT = 1 << 30                    # a confidence counts in units of 2^-30
MAX_KEY = np.uint32(0xFFFFFFFE)   # the saturated score key: as a quantile it admits every class


def _keys(a):
    a = np.ascontiguousarray(_np(a))
    return a.view(np.uint32) if a.dtype == np.int32 else a


def conformal_numpy(pkeys, labels, method="aps", k_reg=0, lam=0.0, coverage=(0.9,), qhat=None):
    """The host restatement of bmi_conformal_scores + bmi_conformal_quantile + bmi_conformal_sets: ``pkeys`` uint32 (or int32) [R, C, N] and
    ``labels`` int32 [N], the classwise records (``classwise_numpy``'s, or the device's first n columns).  Per valid (row, image) — no key
    INVALID, the label in [0, C) —: u_c = (uint64) ((double) conf_c * 2^30); class j precedes class c when key_j > key_c, or key_j == key_c
    and j < c; rank_c and above_c count and sum u over the classes that precede c; score_c = 2^30 - u_c ("lac"), above_c + u_c ("aps"),
    above_c + u_c + floor(lam * 2^30) * max(0, rank_c + 1 - k_reg) ("raps"); the key min(score, 0xFFFFFFFE).  The quantile per row and
    level: k = ceil((n_valid + 1) * coverage), the order statistic of rank k - 1 of the label's keys, 0xFFFFFFFE where k > n_valid.  The
    sets: the classes whose key does not exceed ``qhat`` uint32 [R, L] — the caller's (calibrated elsewhere) or, by default, the one
    formed here.

    Returns dict(class_keys uint32 [R, C, N] (every class's key; INVALID on an invalid pair), score_keys uint32 [R, N], qhat uint32 [R, L],
    n_valid int64 [R], k int64 [R, L], set_size uint8 [R, L, N] (255: invalid), members uint32 [R, L, ceil(C / 32), N], valid int64 [R],
    covered, size_sum int64 [R, L], size_hist, cov_hist int64 [R, L, C + 1], class_n int64 [R, C], class_cov int64 [R, L, C], n).  The walk
    over the classes j is an explicit loop, vectorised over the owned classes c and the images; the integer sums are order-free."""
    keys = _keys(pkeys)
    y = np.asarray(_np(labels)).astype(np.int64).reshape(-1)
    if keys.dtype != np.uint32 or keys.ndim != 3 or y.shape[0] != keys.shape[2]:
        raise ValueError("pkeys uint32 / int32 [R, C, N], labels [N]")
    if method not in METHODS:
        raise ValueError(f"method must be one of {METHODS}, got {method!r}")
    k_reg, lam = int(k_reg), float(lam)
    coverage = tuple(float(q) for q in coverage)
    if k_reg < 0 or not 0.0 <= lam <= 1.0 or not coverage or not all(0.0 < q < 1.0 for q in coverage):
        raise ValueError("k_reg >= 0, lam in [0, 1], coverage levels inside (0, 1)")
    lam_fix = np.uint64(int(lam * 2.0 ** 30))
    R, Cd, N = keys.shape
    L, W = len(coverage), (Cd + 31) // 32
    labelled = (y >= 0) & (y < Cd)
    cls = np.arange(Cd)
    class_keys = np.empty((R, Cd, N), dtype=np.uint32)
    score_keys = np.empty((R, N), dtype=np.uint32)
    ok = np.empty((R, N), dtype=bool)
    for r in range(R):
        ok[r] = labelled & (keys[r] != INVALID).all(axis=0)
        k = np.where(ok[r][None, :], keys[r], 0).astype(np.uint32)                           # a placeholder whose results are dropped
        u = (k.view(np.float32).astype(np.float64) * float(UNIT)).astype(np.uint64)          # truncates
        rank = np.zeros((Cd, N), dtype=np.int64)
        above = np.zeros((Cd, N), dtype=np.uint64)
        for j in range(Cd):                                                                  # the walk
            precedes = (k[j][None, :] > k) | ((k[j][None, :] == k) & (j < cls)[:, None])
            rank += precedes
            above += np.where(precedes, u[j][None, :], np.uint64(0))
        if method == "lac":
            score = np.uint64(UNIT) - u
        else:
            score = above + u
            if method == "raps":
                score = score + lam_fix * np.maximum(rank + 1 - k_reg, 0).astype(np.uint64)
        sk = np.minimum(score, np.uint64(MAX_KEY)).astype(np.uint32)
        class_keys[r] = np.where(ok[r][None, :], sk, INVALID)
        score_keys[r] = np.where(ok[r], sk[np.where(labelled, y, 0), np.arange(N)], INVALID)
    n_valid = ok.sum(axis=1).astype(np.int64)
    kk = np.zeros((R, L), dtype=np.int64)
    own = np.full((R, L), MAX_KEY, dtype=np.uint32)
    for r in range(R):
        line = np.sort(score_keys[r])                                                        # INVALID sorts last
        for l, q in enumerate(coverage):
            kk[r, l] = int(np.ceil(np.float64(n_valid[r] + 1) * np.float64(q)))
            if n_valid[r] > 0 and kk[r, l] <= n_valid[r]:
                own[r, l] = line[kk[r, l] - 1]
    if qhat is None:
        qhat = own
    else:
        qhat = _keys(qhat)
        if qhat.shape != (R, L):
            raise ValueError(f"qhat must be [R, L] = {(R, L)}")
    out = dict(class_keys=class_keys, score_keys=score_keys, qhat=qhat, n_valid=n_valid, k=kk, n=N, valid=n_valid.copy(),
               set_size=np.full((R, L, N), 255, dtype=np.uint8), members=np.zeros((R, L, W, N), dtype=np.uint32),
               covered=np.zeros((R, L), dtype=np.int64), size_sum=np.zeros((R, L), dtype=np.int64),
               size_hist=np.zeros((R, L, Cd + 1), dtype=np.int64), cov_hist=np.zeros((R, L, Cd + 1), dtype=np.int64),
               class_n=np.zeros((R, Cd), dtype=np.int64), class_cov=np.zeros((R, L, Cd), dtype=np.int64))
    for r in range(R):
        v = ok[r]
        yv = y[v]
        out["class_n"][r] = np.bincount(yv, minlength=Cd)
        for l in range(L):
            inside = (class_keys[r] <= qhat[r, l]) & v[None, :]                              # [C, N]
            for c in range(Cd):
                out["members"][r, l, c // 32] |= inside[c].astype(np.uint32) << np.uint32(c % 32)
            size = inside.sum(axis=0)
            hit = inside[np.where(labelled, y, 0), np.arange(N)] & v
            out["set_size"][r, l] = np.where(v, size, 255)
            out["covered"][r, l] = int(hit.sum())
            out["size_sum"][r, l] = int(size[v].sum())
            out["size_hist"][r, l] = np.bincount(size[v], minlength=Cd + 1)
            out["cov_hist"][r, l] = np.bincount(size[hit], minlength=Cd + 1)
            out["class_cov"][r, l] = np.bincount(y[hit], minlength=Cd)
    return out


def conformal_metrics(table):
    """float64 on the host, from the tables of ``MCDEngine.conformal_sets`` or ``conformal_numpy``: dict(coverage [R, L] = covered / valid —
    the marginal coverage —, mean_size [R, L] = size_sum / valid, worst_size_coverage [R, L] = the lowest cov_hist / size_hist over the set
    sizes that occur — the size-stratified coverage of Angelopoulos et al. —, worst_class_coverage [R, L] = the lowest class_cov / class_n
    over the classes that occur, empty [R, L] = the share of empty sets).  A row with ``valid == 0`` gives NaN."""
    t = {k: _np(table[k]).astype(np.int64) for k in ("valid", "covered", "size_sum", "size_hist", "cov_hist", "class_n", "class_cov")}
    with np.errstate(divide="ignore", invalid="ignore"):
        n = t["valid"].astype(np.float64)[:, None]
        by_size = np.where(t["size_hist"] > 0, t["cov_hist"] / t["size_hist"].astype(np.float64), np.inf).min(axis=2)
        by_class = np.where(t["class_n"][:, None, :] > 0, t["class_cov"] / t["class_n"][:, None, :].astype(np.float64), np.inf).min(axis=2)
        return dict(coverage=t["covered"] / n, mean_size=t["size_sum"] / n, empty=t["size_hist"][:, :, 0] / n,
                    worst_size_coverage=np.where(np.isfinite(by_size), by_size, np.nan),
                    worst_class_coverage=np.where(np.isfinite(by_class), by_class, np.nan))


class ConformalAnalysis:
    """Split conformal prediction with the model's engine.  ``fit(calibration_loader)`` walks the loader as ``ReliabilityAnalysis(
    classwise=True)`` does — batch k under seed ``seed + k`` with ``mc_passes`` stochastic passes, the Masksembles counters advanced
    afterwards — into classwise records, forms the calibration scores and stores ``qhat`` int32 [R, L] (device) and ``n_valid`` per exit
    and exit ensemble and per ``coverage`` level.  ``evaluate(test_loader)`` walks a labelled loader the same way and returns the tables of
    ``MCDEngine.conformal_sets`` (with the member words), their ``conformal_metrics`` under ``"metrics"`` and the ``"records"``.
    ``predict(x)`` returns ``set_size`` uint8 [R, L, B] and ``members`` int32 [R, L, ceil(C / 32), B] for one unlabelled batch: it records
    with the dummy label 0 — the classwise record invalidates an image without a label — and returns no coverage figure.  Nothing but the
    quantiles' levels and ``n`` is read on the host.  ``keep_mean=True`` keeps the float64 T-mean probabilities of a walk on the host
    (``fit_mean``, ``evaluate``'s ``"mean"``) beside the labels.  Not under a sharded walk (more than one rank): NotImplementedError."""

    def __init__(self, model, gpu=0, mc_passes=10, seed=0, method="aps", k_reg=0, lam=0.0, coverage=(0.9,), keep_mean=False):
        if method not in METHODS:
            raise ValueError(f"method must be one of {METHODS}, got {method!r}")
        self.model = model
        self.device = get_device(gpu)
        self.mc_passes = int(mc_passes)
        self.seed = seed
        self.score = dict(method=method, k_reg=int(k_reg), lam=float(lam))
        self.coverage = tuple(float(q) for q in coverage)
        self.keep_mean = bool(keep_mean)
        self.qhat = None

    def _engine(self, b_x, loader=None):
        dtype = self.model.resolve_engine_dtype(self.device, None, calib=b_x, samples=self.mc_passes)
        want = max(b_x.shape[0], int(getattr(loader, "batch_size", 0) or 0))
        return self.model.engine(self.device, max_batch=want, dtype=dtype)

    @staticmethod
    def _capacity(loader):
        if getattr(loader, "sampler", None) is not None and hasattr(loader.sampler, "__len__"):
            return len(loader.sampler)
        if hasattr(loader, "dataset"):
            return len(loader.dataset)
        return sum(len(b[0]) for b in loader)

    def _walk(self, loader, labelled=True):
        """(engine, classwise records, n, labels int64 [n], mean float64 [E, n, C] or None) of one walk of ``loader``"""
        import torch
        from ..sharding import _rank_world
        if _rank_world(None)[1] > 1:
            raise NotImplementedError("ConformalAnalysis under a sharded walk: the records are not part of "
                                      "sharding.accumulate_partitioned's all-reduce")
        eng, records, labels, means, off = None, None, [], [], 0
        for k, batch in enumerate(loader):
            b_x = batch[0].to(self.device)
            if eng is None:
                eng = self._engine(b_x, loader)
                records = eng.new_classwise_records(max(1, self._capacity(loader)))
            ml = self.model.mask_layers()
            T, seed, cnt0 = self.mc_passes, self.seed + k, (ml[0].cnt if ml else 0)
            self.model.advance(T)
            mean = eng.predict(b_x, T, seed, cnt0=cnt0)["mean"]
            y = torch.as_tensor(np.asarray(batch[1]).astype(np.int64)) if labelled else torch.zeros(b_x.shape[0], dtype=torch.int64)
            off = eng.classwise_records(mean, y, records, off)
            labels.append(y.numpy())
            if self.keep_mean:
                means.append(mean.cpu().numpy())
        if eng is None:
            raise ValueError("empty loader")
        eng.check_finite()
        return eng, records, off, np.concatenate(labels), (np.concatenate(means, axis=1) if self.keep_mean else None)

    def fit(self, calibration_loader):
        """Walks the labelled calibration loader and stores ``qhat`` int32 [R, L] and ``n_valid`` int64 [R] (device), the ``scores``, the
        records (``fit_records``, ``fit_n``) and ``fit_labels``; returns self."""
        eng, records, n, self.fit_labels, self.fit_mean = self._walk(calibration_loader)
        self.fit_records, self.fit_n = records, n
        self.scores = eng.conformal_scores(records, n, **self.score)
        q = eng.conformal_quantile(self.scores, n, self.coverage)
        self.qhat, self.n_valid = q["qhat"], q["n_valid"]
        return self

    def _sets(self, loader, labelled):
        if self.qhat is None:
            raise RuntimeError("ConformalAnalysis: fit(calibration_loader) comes first")
        eng, records, n, labels, mean = self._walk(loader, labelled)
        out = eng.conformal_sets(records, n, self.qhat, members=True, **self.score)
        out.update(records=records, labels=labels, mean=mean)
        return out

    def evaluate(self, test_loader):
        """Walks the labelled test loader: ``conformal_sets``' dict (with ``members``) plus ``records``, ``labels``, ``mean`` and ``metrics``
        (``conformal_metrics``).  After ``fit``."""
        out = self._sets(test_loader, True)
        out["metrics"] = conformal_metrics(out)
        return out

    def predict(self, x):
        """One unlabelled batch ``x`` [B, 3, 32, 32]: dict(set_size uint8 [R, L, B], members int32 [R, L, ceil(C / 32), B], n).  After ``fit``."""
        out = self._sets([(x, None)], False)
        n = out["n"]
        return dict(set_size=out["set_size"][:, :, :n], members=out["members"][:, :, :, :n], n=n)
