"""Uncertainty decomposition over a loader: the predictive entropy the paper's hardware evaluation reports as aPE (average predictive
entropy, Hardware_Artifact/bayes_hw/metric_utils.py:3-6, computed on random-noise inputs at hls4ml_pred.py:86-119 from
data_utils.py:73-88), and its split into the expected entropy (aleatoric) and the mutual information (epistemic, "BALD") per exit.

The per-sample entropies are summed on the device inside the fused exit head (``MCDEngine.accumulate_uncertainty``); nothing per-sample
reaches memory.  The T-mean probabilities are ``FullAnalysis``'s ``preds`` for the same seed: the walk keeps its per-batch bookkeeping.
"""
import numpy as np

from .results_analyzer import exit_ensembles, get_device


def average_predictive_entropy(p):
    """The reference's aPE of probabilities ``p`` [N, C] (metric_utils.entropy): -sum(log(p + 1e-8) * p) / N."""
    p = np.asarray(p)
    batch_size = p.shape[0]
    return -np.sum(np.log(p + 1e-8) * p) / batch_size


def entropy_rows(p):
    """-sum_c p log p over the last axis, float64, 0 log 0 = 0 (the device's bmi_finalize_uncertainty on the host)."""
    p = np.asarray(p, dtype=np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        t = np.where(p > 0, p * np.log(np.where(p > 0, p, 1.0)), 0.0)
    return -t.sum(axis=-1)


def decompose_logits(logits):
    """The decomposition of per-pass logits [T, ..., C] in float64 on the host (what the device computes from its own per-sample
    logits): dict(mean [..., C], pred_entropy, exp_entropy, mutual_info [...]), entropies in nats, mutual_info clamped at 0."""
    z = np.asarray(logits, dtype=np.float64)
    z = z - z.max(axis=-1, keepdims=True)
    lse = np.log(np.exp(z).sum(axis=-1, keepdims=True))
    p = np.exp(z - lse)
    exp_entropy = (lse[..., 0] - (p * z).sum(axis=-1)).mean(axis=0)
    mean = p.mean(axis=0)
    pred_entropy = entropy_rows(mean)
    return dict(mean=mean, pred_entropy=pred_entropy, exp_entropy=exp_entropy, mutual_info=np.maximum(pred_entropy - exp_entropy, 0.0))


def weighted_exit_ensembles(per_exit, W):
    """Row e = sum_{i<=e} W[e][i] * per_exit[i] for ``per_exit`` [E, ...] and weights ``W`` [E, E], float64: every product rounded, added in
    exit order from 0.0 (the order of csrc/ensemble.hip and of the staged exit rule)."""
    a = np.asarray(per_exit, dtype=np.float64)
    W = np.asarray(W, dtype=np.float64)
    out = np.zeros_like(a)
    for e in range(a.shape[0]):
        for i in range(e + 1):
            out[e] = out[e] + W[e, i] * a[i]
    return out


def calibrated_logits(logits, tau=None, weights=None, scale=None, bias=None, matrix=None):
    """(z, W): the calibrated fp32 logits z [T, E, B, C] of per-pass logits under at most one map — the head's own numbers, as
    ``decompose_ensemble_logits`` states them — and the checked ensemble weights float64 [E, E], or None.  The map is
    ``engine.resolve_calibration_map``'s: a ``tau`` the engines refuse (not finite and > 0) is refused here too."""
    l = np.asarray(logits, dtype=np.float32)
    if l.ndim != 4:
        raise ValueError("logits must be [T, E, B, C]")
    from ..engine import check_ensemble_weights, resolve_calibration_map
    E = l.shape[1]
    m = resolve_calibration_map(tau, scale, bias, matrix, n_exits=E, out_dim=l.shape[3], who="calibrated_logits")
    if m.kind == "temperature":
        inv = (1.0 / np.asarray(m.tau, dtype=np.float64).astype(np.float32).astype(np.float64)).astype(np.float32)
        l = (l * inv[None, :, None, None]).astype(np.float32)
    elif m.kind == "vector":
        l = ((l * m.weight[None, :, None, :]).astype(np.float32) + m.bias[None, :, None, :]).astype(np.float32)
    elif m.kind == "matrix":
        from .calibration import matrix_z
        l = matrix_z(l, m.weight, m.bias)
    W = check_ensemble_weights(weights, E)
    return l, W


def decompose_ensemble_logits(logits, tau=None, weights=None, scale=None, bias=None, matrix=None):
    """The exit ensembles as predictors, from per-pass logits [T, E, B, C] (``MCDEngine.forward_samples``), float64 on the host: the
    definition csrc/ensemble.hip implements on the device (``MCDEngine.predict_ensemble`` / ``ensemble_moments``).  Per pass t the members
    are p_te = softmax(z_te), z = the fp32 logit, or with ``tau`` (a scalar or E temperatures) the tempered head's ONE rounded fp32 product
    float32(l) * float32(1 / tau_e); the ensemble of exits 0..e is q_te = (p_t0 + ... + p_te) / (e + 1) — the reference's per-pass
    ``ensemble += softmax(logits)`` (train/loss/base_classes.py:41,54,58).  Returns dict(mean, var [E, B, C] — var with ddof 0, clamped at
    0 —, pred_entropy H[mean], exp_entropy E_t H[q_t], mutual_info [E, B] — clamped at 0), entropies in nats.  Row 0 is exit 0 itself.
    The exits of one pass share the trunk's draw: ``var`` is NOT sum_i var_i / (e + 1)^2.  ``weights`` (None, [E] or [E, E]:
    ``engine.check_ensemble_weights``): the weighted ensembles q_te = ((W[e][0] p_t0 + W[e][1] p_t1) + ...) + W[e][e] p_te — every product
    rounded, added in exit order from 0.0, no renormalisation — in place of the equal mean; everything behind q is the same.  ``scale`` /
    ``bias`` (``engine.check_vector_scaling``: [E, C] or [C], bias None = zeros; not together with ``tau``): the members under a vector
    scaling, z = float32(float32(l * scale) + bias), the vector-scaled head's two rounded fp32 operations.  ``matrix`` / ``bias``
    (``engine.check_matrix_scaling``; not together with ``tau`` or ``scale``): the members under a matrix scaling, z = the fp32 number of
    ``train.calibration.matrix_z``."""
    l, W = calibrated_logits(logits, tau, weights, scale, bias, matrix)
    T, E = l.shape[:2]
    z = l.astype(np.float64)
    z = z - z.max(axis=-1, keepdims=True)
    ex = np.exp(z)
    p = ex / ex.sum(axis=-1, keepdims=True)
    q1 = np.zeros(l.shape[1:], dtype=np.float64)
    q2 = np.zeros(l.shape[1:], dtype=np.float64)
    qh = np.zeros(l.shape[1:3], dtype=np.float64)
    for t in range(T):                          # in sample order onto the running sums, like the device
        acc = np.zeros(l.shape[2:], dtype=np.float64)
        qw = None if W is None else weighted_exit_ensembles(p[t], W)
        for e in range(E):
            acc = acc + p[t, e]
            q = acc / (e + 1) if W is None else qw[e]
            q1[e] += q
            q2[e] += q * q
            qh[e] += entropy_rows(q)
    mean = q1 / T
    var = np.maximum(q2 / T - mean * mean, 0.0)
    pred_entropy = entropy_rows(mean)
    exp_entropy = qh / T
    return dict(mean=mean, var=var, pred_entropy=pred_entropy, exp_entropy=exp_entropy,
                mutual_info=np.maximum(pred_entropy - exp_entropy, 0.0))


def vote_counts_numpy(logits, tau=None, weights=None, scale=None, bias=None, matrix=None, rows=None, n_e=None):
    """The vote counts of per-pass logits [T, E, B, C] on the host: the definition csrc/votes.hip implements on the device
    (``MCDEngine.accumulate_votes`` / ``vote_counts``).  z = the calibrated fp32 logits of ``decompose_ensemble_logits`` (same arguments);
    a row (t, e, b) with a non-finite z is bad.  V[0, e, b, k] counts the passes whose row is not bad and whose lowest arg-max of z (fp32
    comparisons) is k; V[1, e, b, k] the passes with no bad row among exits 0..e whose lowest arg-max of the float64 exit ensemble q_te —
    (p_t0 + ... + p_te) / (e + 1), or the weighted sum in exit order from 0.0 — is k.  Returns (V int32 [2, E, B, C], the number of bad
    rows).  ``rows`` (image indices) and ``n_e`` (int [B]): the image-list form of csrc/votes_rows.hip (``MCDEngine.vote_counts(rows=,
    n_exits_of_image=)``) — only the listed images, and of image b only the exits e < n_e[b], are looked at: their counts are the full
    form's (the running exit sum is cut, not changed), every other row of V is zero and a bad row there is not counted."""
    l, W = calibrated_logits(logits, tau, weights, scale, bias, matrix)
    T, E, B, Cd = l.shape
    use = np.ones((E, B), dtype=bool)                                    # the (exit, image) rows the call looks at
    if rows is not None:
        use[:] = False
        use[:, np.asarray(rows, dtype=np.int64)] = True
    if n_e is not None:
        use &= np.arange(E)[:, None] < np.asarray(n_e, dtype=np.int64)[None, :]
    l = np.where(use[None, :, :, None], l, np.float32(0))                # (rows not looked at: a finite placeholder nobody counts)
    bad = ~np.isfinite(l).all(axis=-1)                                   # [T, E, B]
    ens_bad = np.cumsum(bad, axis=1) > 0
    with np.errstate(invalid="ignore", over="ignore"):
        z = np.where(bad[..., None], 0.0, l.astype(np.float64))          # (bad rows: a placeholder nobody counts)
        z = z - z.max(axis=-1, keepdims=True)
        ex = np.exp(z)
        p = ex / ex.sum(axis=-1, keepdims=True)
    V = np.zeros((2, E, B, Cd), dtype=np.int32)
    imgs = np.arange(B)
    for t in range(T):
        k = np.where(bad[t][..., None], -np.inf, l[t]).argmax(axis=-1)   # [E, B]: numpy's argmax is the first maximum
        acc = np.zeros((B, Cd), dtype=np.float64)
        qw = None if W is None else weighted_exit_ensembles(p[t], W)
        for e in range(E):
            acc = acc + p[t, e]
            q = acc / (e + 1) if W is None else qw[e]
            ok = ~bad[t, e] & use[e]
            np.add.at(V[0, e], (imgs[ok], k[e][ok]), 1)
            ok = ~ens_bad[t, e] & use[e]
            np.add.at(V[1, e], (imgs[ok], q.argmax(axis=-1)[ok]), 1)
    return V, int(bad.sum())


def vote_decided_numpy(V_row, t, T_max, slack=0):
    """The decided-vote stop rule (BMI_STOP_VOTES; csrc/votes_rows.hip: vote_decide_kernel) on the host, integers only: ``V_row`` int
    [..., C] = the counts of one row of V after ``t`` of ``T_max`` passes.  c1 = the lowest class with the largest count, lead = min over
    c != c1 of V[c1] - V[c] - (1 if c < c1 else 0) — a class below c1 wins a tie — or INT32_MAX when C == 1; decided = lead >=
    max(0, T_max - t - slack).  With slack 0 a decided row's lowest arg-max cannot change in the passes still to come, whatever they
    vote.  Returns (decided bool [...], lead int64 [...])."""
    V = np.asarray(V_row).astype(np.int64)
    Cd = V.shape[-1]
    c1 = V.argmax(axis=-1)                                               # numpy's argmax is the first maximum
    top = np.take_along_axis(V, c1[..., None], axis=-1)
    c = np.arange(Cd)
    gap = top - V - (c < c1[..., None])
    gap = np.where(c == c1[..., None], np.iinfo(np.int32).max, gap)
    lead = gap.min(axis=-1)
    return lead >= max(0, int(T_max) - int(t) - int(slack)), lead


def vote_readout_numpy(V):
    """The read-out of vote counts V [..., C] (bmi_finalize_votes on the host): dict(vote_class int32 — the lowest class with the modal
    count, -1 where no vote was cast —, variation_ratio = 1 - modal count / votes cast (1.0 where none), vote_entropy = -sum f log f over
    the classes with votes, subtracted in class order from 0.0, in nats (0.0 where none)), each [...]."""
    V = np.asarray(V)
    n = V.sum(axis=-1, dtype=np.int64)
    m = V.max(axis=-1)
    some = n > 0
    nn = np.where(some, n, 1).astype(np.float64)
    h = np.zeros(n.shape, dtype=np.float64)
    for c in range(V.shape[-1]):
        x = V[..., c]
        f = x.astype(np.float64) / nn
        h = h - np.where(x > 0, f * np.log(np.where(x > 0, f, 1.0)), 0.0)
    return dict(vote_class=np.where(some, V.argmax(axis=-1), -1).astype(np.int32),
                variation_ratio=np.where(some, 1.0 - m.astype(np.float64) / nn, 1.0), vote_entropy=np.where(some, h, 0.0))


class UncertaintyAnalysis:
    """One walk of ``loader`` (batches ``(x, y, ...)``) with ``mc_passes`` stochastic passes per batch.

    Batch k runs under seed ``seed + k`` with the model's current Masksembles counter, and the counters advance by ``mc_passes``
    afterwards: the bookkeeping of ``FullAnalysis._batch_call``, so ``mean`` equals ``FullAnalysis(model, loader, mc_dropout=True,
    mc_passes=T, seed=seed).preds``.  The engine is the model's (``engine_dtype="auto"`` applies).  Under an initialised
    ``torch.distributed`` with more than one rank every rank walks the same loader and each batch is partitioned like ``FullAnalysis``'s
    (``sharding.predict_sharded_uncertainty``: one all-reduce per batch); every rank ends with the full arrays, rank 0 writes them.

    Per exit, float64: ``mean`` [E, N, C], ``pred_entropy`` / ``exp_entropy`` / ``mutual_info`` [E, N]; ``ape`` [E] (the reference's
    aPE of the T-mean probabilities), ``mean_mi`` [E], ``mean_exp_entropy`` [E]; ``ensemble_pred_entropy`` [E, N] and ``ensemble_ape``
    [E]: the same for the reference's cumulative exit ensembles (the mean of exits 0..e).

    ``ensemble=True``: the walk treats every exit ensemble as a predictor of its own (``MCDEngine.predict_ensemble``: the per-sample
    ensembles are accumulated on the device) and also fills ``ensemble_var`` [E, N, C], ``ensemble_exp_entropy`` and
    ``ensemble_mutual_info`` [E, N], ``ensemble_mean_mi`` [E]; ``summary()`` and ``save()`` gain those keys.  ``ensemble_pred_entropy`` is then the
    device's entropy of the float64 ensemble mean (within 1e-5 of the default walk's, whose members are the heads' fp32 softmax), so that
    ensemble_mutual_info = ensemble_pred_entropy - ensemble_exp_entropy; everything else keeps its numbers.  Not under a sharded walk (more than one rank): NotImplementedError.
    On a model that carries ensemble weights (``set_exit_ensemble_weights``) the ``ensemble=True`` walk describes the WEIGHTED ensembles —
    the five device arrays through the engine, ``ensemble_ape`` from the weighted mean of ``mean``; the default walk keeps the equal mean.

    ``votes=True`` (implies ``ensemble=True``; not under a sharded walk either): the walk also counts every pass's votes on the device
    (``MCDEngine.predict_votes``) and fills ``votes`` int32 [E, N, C], ``vote_class`` int32 [E, N] (the majority vote), ``variation_ratio`` and
    ``vote_entropy`` [E, N], their ``ensemble_*`` twins for the exit ensembles, ``mean_variation_ratio`` [E] and ``vote_agreement`` [E], the
    share of images whose majority vote equals the arg-max of ``mean`` (``ensemble_mean_variation_ratio`` / ``ensemble_vote_agreement``:
    the same against the device's ensemble mean); ``summary()`` and ``save()`` gain those keys.  Every attribute of the ``ensemble=True``
    walk keeps its numbers."""

    VOTE_KEYS = ("votes", "vote_class", "variation_ratio", "vote_entropy")

    def __init__(self, model, loader, gpu=0, mc_passes=10, seed=0, group=None, ensemble=False, votes=False):
        self.count_votes = bool(votes)               # (``votes`` itself becomes the array of counts)
        self.ensemble = bool(ensemble) or self.count_votes
        self.model = model
        self.loader = loader
        self.device = get_device(gpu)
        self.mc_passes = int(mc_passes)
        self.seed = seed
        self.group = group
        self._run()

    def _ranks(self):
        from ..sharding import _rank_world
        return _rank_world(self.group)

    def is_writer(self):
        return self._ranks()[0] == 0

    def _engine(self, b_x):
        dtype = self.model.resolve_engine_dtype(self.device, None, calib=b_x, samples=self.mc_passes)
        if self._ranks()[1] > 1:          # (collective: every rank builds its engine on the same first batch)
            import torch.distributed as dist
            dtype = self.model.agree_engine_dtype(self.device, dtype, self.group or dist.group.WORLD)
        want = max(b_x.shape[0], int(getattr(self.loader, "batch_size", 0) or 0))
        return self.model.engine(self.device, max_batch=want, dtype=dtype)

    def _run(self):
        from ..sharding import predict_sharded_uncertainty
        world = self._ranks()[1]
        if self.count_votes and world > 1:
            raise NotImplementedError("UncertaintyAnalysis(votes=True) under a sharded walk: the vote counts are not part of "
                                      "sharding.accumulate_partitioned's all-reduce")
        if self.ensemble and world > 1:
            raise NotImplementedError("UncertaintyAnalysis(ensemble=True) under a sharded walk: the ensemble sums are not part of "
                                      "sharding.accumulate_partitioned's all-reduce")
        names = ("mean", "pred_entropy", "exp_entropy", "mutual_info")
        if self.ensemble:
            names += ("ens_var", "ens_pred_entropy", "ens_exp_entropy", "ens_mutual_info")
        if self.count_votes:
            names += ("ens_mean",) + self.VOTE_KEYS + tuple("ens_" + n for n in self.VOTE_KEYS)
        parts, labels, eng = [], [], None
        for k, batch in enumerate(self.loader):
            b_x = batch[0].to(self.device)
            if eng is None:
                eng = self._engine(b_x)
            ml = self.model.mask_layers()
            T, seed, cnt0 = self.mc_passes, self.seed + k, (ml[0].cnt if ml else 0)
            self.model.advance(T)
            if world > 1:
                r = predict_sharded_uncertainty(eng, b_x, T, seed, cnt0, group=self.group)
            elif self.count_votes:
                r = eng.predict_votes(b_x, T, seed, cnt0=cnt0)
            elif self.ensemble:
                r = eng.predict_ensemble(b_x, T, seed, cnt0=cnt0)
            else:
                r = eng.predict_uncertainty(b_x, T, seed, cnt0=cnt0)
            parts.append({n: r[n].cpu().numpy() for n in names})
            eng.check_finite()
            labels.append(np.asarray(batch[1]).astype(np.int64))
        if not parts:
            raise ValueError("empty loader")
        self.mean = np.concatenate([p["mean"] for p in parts], axis=1)
        self.pred_entropy = np.concatenate([p["pred_entropy"] for p in parts], axis=1)
        self.exp_entropy = np.concatenate([p["exp_entropy"] for p in parts], axis=1)
        self.mutual_info = np.concatenate([p["mutual_info"] for p in parts], axis=1)
        self.labels = np.concatenate(labels)
        self.ape = np.array([average_predictive_entropy(m) for m in self.mean])
        self.mean_mi = self.mutual_info.mean(axis=1)
        self.mean_exp_entropy = self.exp_entropy.mean(axis=1)
        W = getattr(self.model, "exit_ensemble_weights", None) if self.ensemble else None
        ens = exit_ensembles(self.mean) if W is None else weighted_exit_ensembles(self.mean, W)
        self.ensemble_pred_entropy = entropy_rows(ens)
        self.ensemble_ape = np.array([average_predictive_entropy(m) for m in ens])
        if self.ensemble:
            # the device's H[ens_mean] (float64 softmax members; the line above: the heads' fp32 ones): ensemble_mutual_info is ITS difference
            self.ensemble_pred_entropy = np.concatenate([p["ens_pred_entropy"] for p in parts], axis=1)
            self.ensemble_var = np.concatenate([p["ens_var"] for p in parts], axis=1)
            self.ensemble_exp_entropy = np.concatenate([p["ens_exp_entropy"] for p in parts], axis=1)
            self.ensemble_mutual_info = np.concatenate([p["ens_mutual_info"] for p in parts], axis=1)
            self.ensemble_mean_mi = self.ensemble_mutual_info.mean(axis=1)
        if self.count_votes:
            for n in self.VOTE_KEYS:
                setattr(self, n, np.concatenate([p[n] for p in parts], axis=1))
                setattr(self, "ensemble_" + n, np.concatenate([p["ens_" + n] for p in parts], axis=1))
            ens_mean = np.concatenate([p["ens_mean"] for p in parts], axis=1)
            self.mean_variation_ratio = self.variation_ratio.mean(axis=1)
            self.ensemble_mean_variation_ratio = self.ensemble_variation_ratio.mean(axis=1)
            self.vote_agreement = (self.vote_class == self.mean.argmax(axis=-1)).mean(axis=1)
            self.ensemble_vote_agreement = (self.ensemble_vote_class == ens_mean.argmax(axis=-1)).mean(axis=1)

    def _vote_arrays(self):
        names = self.VOTE_KEYS + tuple("ensemble_" + n for n in self.VOTE_KEYS) + \
            ("mean_variation_ratio", "ensemble_mean_variation_ratio", "vote_agreement", "ensemble_vote_agreement")
        return {n: getattr(self, n) for n in names}

    def summary(self):
        """Per exit: dict(ape, mean_mi, mean_exp_entropy, ensemble_ape), ensemble_mean_mi of an ``ensemble=True`` walk, and the mean
        variation ratios and vote agreements of a ``votes=True`` walk."""
        out = [dict(ape=float(self.ape[e]), mean_mi=float(self.mean_mi[e]), mean_exp_entropy=float(self.mean_exp_entropy[e]),
                    ensemble_ape=float(self.ensemble_ape[e])) for e in range(len(self.ape))]
        if self.ensemble:
            for e, d in enumerate(out):
                d["ensemble_mean_mi"] = float(self.ensemble_mean_mi[e])
        if self.count_votes:
            for e, d in enumerate(out):
                for n in ("mean_variation_ratio", "ensemble_mean_variation_ratio", "vote_agreement", "ensemble_vote_agreement"):
                    d[n] = float(getattr(self, n)[e])
        return out

    def save(self, experiment_id):
        """``test_uncertainty_<experiment_id>.npz`` (rank 0 of a sharded walk only); returns the file name, or None on the other ranks."""
        if not self.is_writer():
            return None
        name = f"test_uncertainty_{experiment_id}.npz"
        extra = {}
        if self.ensemble:
            extra = dict(ensemble_var=self.ensemble_var, ensemble_exp_entropy=self.ensemble_exp_entropy,
                         ensemble_mutual_info=self.ensemble_mutual_info, ensemble_mean_mi=self.ensemble_mean_mi)
        if self.count_votes:
            extra.update(self._vote_arrays())
        np.savez(name, mean=self.mean, pred_entropy=self.pred_entropy, exp_entropy=self.exp_entropy, mutual_info=self.mutual_info,
                 labels=self.labels, ape=self.ape, mean_mi=self.mean_mi, mean_exp_entropy=self.mean_exp_entropy,
                 ensemble_pred_entropy=self.ensemble_pred_entropy, ensemble_ape=self.ensemble_ape, **extra)
        return name
