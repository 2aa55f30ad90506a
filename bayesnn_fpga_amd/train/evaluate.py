"""Mirror of SA/train/evaluate.py:8-22 (MCD use #1): T OUTER passes over the whole loader, each pass
computing the multi-exit accuracy vector (SA/train/loss/base_classes.py:39-66), averaged over T.
Every ``model(X)`` is one stochastic pass on the GPU; the accuracy arithmetic is host collation."""
import numpy as np
import torch
import torch.nn.functional as F

from .results_analyzer import get_device


class MultiExitAccuracy:
    """``_MultiExitAccuracy`` (base_classes.py:22-70) incl. its row-0 overwrite quirk (:45-48)."""

    def __init__(self, n_exits, acc_tops=(1, 5)):
        self.n_exits, self._acc_tops = n_exits, tuple(acc_tops)
        self.metric_names = [f"acc{i}_avg" for i in acc_tops]
        for i in acc_tops:
            self.metric_names += [f"acc{i}_clf{k}" for k in range(n_exits)]
            self.metric_names += [f"acc{i}_ens{k}" for k in range(1, n_exits)]
        self.metric_names += ["avg_maxprob"]

    defer_host_sync = True      # validate_model_acc keeps the metric vectors of a loader walk on the device (False: .cpu() per batch)

    def _topk(self, scores, y):
        _, pred = scores.topk(k=max(self._acc_tops), dim=1)
        hit = (pred == y[:, None]).float().cumsum(dim=1).mean(dim=0)
        return hit[[i - 1 for i in self._acc_tops]]

    def _metrics_tensor(self, logits_list, y):
        """The metric vector as ONE fp32 device tensor (same arithmetic, same order as the reference's ``_metrics``): no host
        synchronisation, so the batches of a loader walk queue up behind each other on the GPU."""
        k = len(self._acc_tops)
        ensemble = torch.zeros_like(logits_list[0])
        acc_clf = torch.zeros(self.n_exits, k, device=y.device)
        acc_ens = torch.zeros(self.n_exits, k, device=y.device)
        last = len(logits_list) - 1
        for i, logits in enumerate(logits_list):
            if self.n_exits == 1 and i != last:
                continue
            ensemble += F.softmax(logits, dim=1)
            if i == last:                           # reference quirk (`i = 0`, base_classes.py:45-48): every exit writes row 0, so only the
                acc_clf[0] = self._topk(logits, y)  # last exit's accuracies and the full ensemble's survive — the overwritten top-k's
                acc_ens[0] = self._topk(ensemble, y)    # (six small launches per exit) are not computed
        maxprob = F.softmax(logits_list[-1], dim=1).max(dim=1)[0].mean()
        # (the reference averages the per-exit rows in numpy float64: np.zeros(...).mean(axis=0))
        parts = [acc_clf.double().mean(dim=0)]
        for i in range(k):
            parts += [acc_clf[:, i].double(), acc_ens[1:, i].double()]
        return torch.cat(parts + [maxprob.double()[None]])

    def _metrics(self, logits_list, y):
        return [float(v) for v in self._metrics_tensor(logits_list, y).cpu()]

    def _metrics_passes(self, logits, y):
        """``_metrics_tensor`` for T passes at once: ``logits`` fp32 [T, E, B, C] (MCDEngine.forward_samples) -> float64 [T, n_metrics],
        row i = the vector ``_metrics`` gives for pass i's logits list (same arithmetic per pass, batched over T on the device).
        With a leading group axis — ``logits`` [G, T, E, B, C], ``y`` [G, B]: G batches of one size — [G, T, n_metrics]: the metric
        arithmetic of a whole group of loader batches in a dozen launches."""
        grouped = logits.dim() == 5
        if not grouped:
            logits, y = logits[None], y[None]
        G, T, E, Bn, C = logits.shape
        k = len(self._acc_tops)
        probs = F.softmax(logits if self.n_exits > 1 else logits[:, :, -1:], dim=-1)    # n_exits == 1: only the last logits count
        ensemble = probs[:, :, 0].clone()
        for i in range(1, probs.shape[2]):
            ensemble += probs[:, :, i]                       # (the reference's order: exit 0 first)
        both = torch.stack([logits[:, :, -1], ensemble])    # [2, G, T, B, C]: the two rows of the reference's quirk that survive
        _, pred = both.topk(k=max(self._acc_tops), dim=-1)
        hit = (pred == y[None, :, None, :, None]).float().cumsum(dim=-1).mean(dim=3)[..., [i - 1 for i in self._acc_tops]]   # [2, G, T, k]
        acc_clf = torch.zeros(G, T, self.n_exits, k, device=y.device)
        acc_ens = torch.zeros(G, T, self.n_exits, k, device=y.device)
        acc_clf[:, :, 0] = hit[0]                            # (the reference's row-0 overwrite: the last exit and the full ensemble survive)
        acc_ens[:, :, 0] = hit[1]
        maxprob = probs[:, :, -1].max(dim=-1)[0].mean(dim=-1)
        parts = [acc_clf.double().mean(dim=2)]
        for i in range(k):
            parts += [acc_clf[..., i].double(), acc_ens[:, :, 1:, i].double()]
        out = torch.cat(parts + [maxprob.double()[..., None]], dim=-1)
        return out if grouped else out[0]

    def metrics(self, net, X, y):
        return self._metrics(net.train(False)(X), y)


def validate_model_acc(loss_f, net, val_iter, gpu):
    """SA/train/train_utils.py:32-38.  Every ``net(X)`` is one stochastic pass on the GPU (asynchronous on the current stream); the
    metric vectors of the batches stay on the device until the walk is over — ONE host synchronisation per pass over the loader
    instead of nine per batch (the reference's ``.cpu()`` per top-k: SA/train/loss/base_classes.py:58-62), the same numbers."""
    dev = get_device(gpu)
    if getattr(loss_f, "defer_host_sync", False):
        net.train(False)
        rows = torch.stack([loss_f._metrics_tensor(net(X.to(dev, non_blocking=True)), y.to(dev, non_blocking=True)) for X, y in val_iter]).cpu()
        rows = [[float(v) for v in r] for r in rows]
    else:
        rows = [loss_f.metrics(net, X.to(dev), y.to(dev)) for X, y in val_iter]
    return [sum(col) / len(col) for col in zip(*rows)]


def _eval_pipe(model, dev, dtype, batch):
    """The folded evaluation's two engines in flight for (device, dtype), ONE per key: a batch larger than the pipe was built for replaces it —
    the old engines are closed, their workspaces dropped (like ``EngineModelMixin.engine()`` grows) — so successive evaluations with growing
    batch sizes, or a loader whose first batch is small, never accumulate workspaces.  ``model.invalidate_engine()`` / ``.to()`` /
    ``load_state_dict`` clear the cache: after in-place weight updates call ``invalidate_engine()`` before the next evaluate()."""
    from ..engine import BatchesInFlight
    pipes = model.__dict__.setdefault("_eval_pipes", {})
    key = (str(dev), dtype)
    pipe = pipes.get(key)
    if pipe is not None and pipe.engines and pipe.engines[0].max_batch >= batch:
        return pipe
    if pipe is not None:
        pipe.close()
    pipe = pipes[key] = BatchesInFlight(model, dev, n=2, max_batch=batch, dtype=dtype)
    return pipe


class _TorchReadout:
    """The read-out of a folded walk through torch (``MultiExitAccuracy._metrics_passes``): the engine passes write their logits into ONE
    group buffer [G, T, E, B, C] (<= 256 MB), and the metric arithmetic runs once per group: per batch, its dozen tiny launches queued
    between the other stream's convolutions cost 0.7 ms of a 3.2 ms batch (tools/experiments/evaluate_fold_profile.py)."""

    def __init__(self, loss_fn, dev):
        self.loss_fn, self.dev = loss_fn, dev
        self.rows, self.group_buf = [], None              # group_buf = [logits buffer, labels, batches filled, capacity, batch size]

    def flush(self, pipe, dtype):
        group_buf = self.group_buf
        if group_buf is not None and group_buf[2]:
            pipe.synchronize()
            lg = group_buf[0][:group_buf[2]]
            if not bool(torch.isfinite(lg).all()):     # (a 16-bit overflow: inf / NaN logits would turn into plausible-looking accuracies)
                raise FloatingPointError(f"non-finite logits on the {dtype!r} engine: use engine_dtype='f16x2' / 'bf16x3' (or 'auto')")
            self.rows.append(self.loss_fn._metrics_passes(lg, torch.stack(group_buf[1])))
        self.group_buf = None

    def batch(self, pipe, dtype, k, nb, Tl, Xd, yd, forward):
        Bk = int(Xd.shape[0])
        if self.group_buf is not None and (self.group_buf[4] != Bk or self.group_buf[2] == self.group_buf[3]):
            self.flush(pipe, dtype)
        if self.group_buf is None:
            e0 = pipe.engines[0]
            cap = max(1, min(nb - k, (1 << 28) // (Tl * e0.n_exits * Bk * e0.out_dim * 4)))
            self.group_buf = [torch.empty(cap, Tl, e0.n_exits, Bk, e0.out_dim, dtype=torch.float32, device=self.dev), [], 0, cap, Bk]
        group_buf = self.group_buf
        slot = group_buf[0][group_buf[2]]
        group_buf[1].append(yd)
        group_buf[2] += 1
        pipe.submit(lambda eng, slot=slot: forward(eng, slot), inputs=(Xd,))

    def table(self, nb, T, t_lo, t_hi):
        """[n_batches, T, n_metrics] float64 on the device, this rank's passes filled in"""
        per_batch = torch.zeros(nb, T, len(self.loss_fn.metric_names), dtype=torch.float64, device=self.dev)
        if self.rows:
            per_batch[:, t_lo:t_hi] = torch.cat(self.rows)
        return per_batch


class _DeviceReadout:
    """The read-out of a folded walk on the device (``MCDEngine.pass_accuracy``): every batch's ``forward_samples`` goes into a logits
    buffer of the engine that runs it, ONE bmi_pass_accuracy call follows on the same engine and stream and writes row k of the
    [n_batches, T_local, ...] count tables; nothing per sample is kept beyond that buffer.  The non-finite counter of the kernel takes the
    place of the ``torch.isfinite`` pass over the logits.  ``columns(hits, maxprob, Bs)`` turns the tables (host arrays, after the walk's
    one synchronisation) into the [n_batches, T_local, n_columns] float64 rows of the caller's metric table."""

    def __init__(self, tops, dev, columns, n_columns):
        self.tops, self.dev, self.columns, self.n_columns = tuple(int(i) for i in tops), dev, columns, n_columns
        self.hits = self.maxprob = self.nonfinite = None
        self.sizes, self.pipe, self.dtype = {}, None, None

    def flush(self, pipe, dtype):
        pass                                                # (nothing is grouped: the tables outlive a pipe that is replaced)

    def batch(self, pipe, dtype, k, nb, Tl, Xd, yd, forward):
        e0 = pipe.engines[0]
        E, Cd, Bk = e0.n_exits, e0.out_dim, int(Xd.shape[0])
        if self.hits is None:
            self.hits = torch.zeros(nb, Tl, 2, E, len(self.tops), dtype=torch.int32, device=self.dev)
            self.maxprob = torch.zeros(nb, Tl, E, dtype=torch.float64, device=self.dev)
            self.nonfinite = torch.zeros(1, dtype=torch.int32, device=self.dev)
        self.sizes[k], self.pipe, self.dtype = Bk, pipe, dtype
        out, nf, tops = (self.hits[k], self.maxprob[k]), self.nonfinite, self.tops

        def run(eng):
            lg = eng._scratch("_eval_logits", Tl * E * Bk * Cd * 4)[:Tl * E * Bk * Cd * 4].view(torch.float32).view(Tl, E, Bk, Cd)
            forward(eng, lg)
            eng.pass_accuracy(lg, yd, tops, out=out, nonfinite=nf)
        pipe.submit(run, inputs=(Xd, yd))

    def table(self, nb, T, t_lo, t_hi):
        """[n_batches, T, n_columns] float64 on the HOST, this rank's passes filled in"""
        per_batch = torch.zeros(nb, T, self.n_columns, dtype=torch.float64)
        if self.hits is not None:
            self.pipe.synchronize()
            if int(self.nonfinite.item()):                  # (a 16-bit overflow: inf / NaN logits would turn into plausible-looking accuracies)
                raise FloatingPointError(f"non-finite logits on the {self.dtype!r} engine: use engine_dtype='f16x2' / 'bf16x3' (or 'auto')")
            Bs = np.array([self.sizes.get(k, 1) for k in range(nb)], dtype=np.int64)
            per_batch[:, t_lo:t_hi] = torch.from_numpy(self.columns(self.hits.cpu().numpy(), self.maxprob.cpu().numpy(), Bs))
        return per_batch


def _walk_folded(readout, test_iter, model, dev, T, group=None, shard=None):
    """The T outer passes of evaluate() FOLDED per batch: one walk over the loader, every batch's T stochastic forwards as ONE pass of
    the engine (``MCDEngine.forward_samples``: prefix once, samples folded into the launches) and the metric rows of its T passes from
    ``readout`` (``_TorchReadout``: one batched device op per group of batches; ``_DeviceReadout``: one kernel call per batch).  What the
    reference's loop order fixes is reproduced: pass i of batch k of an n-batch loader
    is forward call i n + k, so its Masksembles mask is (cnt + k + i n) mod M (``mask_stride`` = n) and the layers' counters — and the
    mirror's MC pass index — end T n calls further.  MC-dropout masks are i.i.d. draws addressed by the sample index: pass i of batch k
    takes index mc_pass + k T + i here (the unfolded walk numbers them in call order, mc_pass + i n + k: another labelling of the same
    draws — the averaged metrics agree in distribution, not sample for sample).

    MULTI-GPU: under an initialised ``torch.distributed`` with more than one rank (``shard=None``: automatic) every rank walks
    the same loader and runs passes [lo, hi) of every batch (``sharding.shard_range`` over T: the T samples shard across the GPUs); the
    per-pass metric rows are disjoint, ONE all-reduce (sum) of the [n_batches, T, n_metrics] float64 table at the end of the walk joins them,
    and every rank holds the same table.  Returns it as a host array [n_batches, T, n_metrics]."""
    from ..sharding import _rank_world, shard_range
    nb = len(test_iter)
    cnt = model.mask_layers()[0].cnt if model.mask_layers() else 0
    rank, world = (0, 1) if shard is False else _rank_world(group)
    t_lo, t_hi = shard_range(T, rank, world)
    Tl = t_hi - t_lo                                    # this rank's passes (0: more ranks than passes — it only takes part in the all-reduce)
    # Two batches in flight (engine.BatchesInFlight: own engine, workspace and stream each): the host-to-device copy of one batch runs
    # beside the engine pass of the other.
    pipe, dtype = None, None
    for k, (X, y) in enumerate(test_iter):
        Bk = int(X.shape[0])
        Xd, yd = X.to(dev, non_blocking=True), y.to(dev, non_blocking=True)      # (on the caller's stream: the slot's stream waits for it)
        if dtype is None:
            dtype = model.resolve_engine_dtype(dev, None, calib=Xd, samples=T)   # engine_dtype = "auto": decided on the first batch, at the caller's T
            if world > 1:            # (collective, on every rank's first batch — also a rank without passes of its own)
                dtype = model.agree_engine_dtype(dev, dtype, group)
        if Tl == 0:
            continue
        if pipe is None or pipe.engines[0].max_batch < Bk:
            readout.flush(pipe, dtype)
            pipe = _eval_pipe(model, dev, dtype, Bk)
        readout.batch(pipe, dtype, k, nb, Tl, Xd, yd,
                      lambda eng, out, Xd=Xd, k=k: eng.forward_samples(Xd, Tl, seed=model.mc_seed, t_begin=model.mc_pass + k * T + t_lo,
                                                                       cnt0=cnt + k + t_lo * nb, mask_stride=nb, out=out))
    readout.flush(pipe, dtype)
    per_batch = readout.table(nb, T, t_lo, t_hi)
    model.advance(T * nb)
    if world > 1:
        import torch.distributed as dist
        if dist.get_backend(group) == "nccl":
            per_batch = per_batch.to(dev)
            dist.all_reduce(per_batch, op=dist.ReduceOp.SUM, group=group)
        else:                                           # (gloo: the CPU tests and the two-ranks-on-one-GPU dry run)
            host = per_batch.cpu()
            dist.all_reduce(host, op=dist.ReduceOp.SUM, group=group)
            per_batch = host
    return per_batch.cpu().numpy()                      # [n_batches, T, n_metrics]: one host synchronisation per group of batches


def _per_pass(per_batch):
    """per pass: sum over the batches in loader order / n (train_utils.py:38), in Python floats like the reference"""
    nb, T = per_batch.shape[:2]
    return np.array([[sum(float(per_batch[k, i, j]) for k in range(nb)) / nb for j in range(per_batch.shape[2])] for i in range(T)])


def _fraction(count, B, gpu_mean=True):
    """A hit count over the batch size as torch's fp32 ``mean`` of 0 / 1 values gives it, widened to double.  On the GPU — where the torch
    route and the reference form it — the reduction multiplies the (exact) sum by its factor: float32(count) * float32(1 / B); torch's
    CPU mean divides: float32(count) / float32(B) (``gpu_mean=False``).  The two agree whenever B is a power of two."""
    c, n = np.asarray(count).astype(np.float32), np.asarray(B).astype(np.float32)
    return (c * (np.float32(1) / n) if gpu_mean else c / n).astype(np.float64)


def metric_rows_from_counts(loss_fn, hits, maxprob, B, gpu_mean=True):
    """The reference's metric vector (``MultiExitAccuracy._metrics_passes``, row-0 overwrite included) from the counts of
    ``pass_accuracy``: ``hits`` int [..., 2, E, K], ``maxprob`` float64 [..., E], ``B`` the batch size, broadcast against the leading
    axes -> float64 [..., n_metrics].  Of the 2 E rows only the last exit's survives in the vector (as row clf0; the full ensemble lands
    in a row the reference never emits): acc{i}_clf0 = the count over B as torch's fp32 mean forms it (``_fraction``: on the GPU by default,
    ``gpu_mean=False``: on the CPU), acc{i}_avg = that / n_exits, avg_maxprob = maxprob[E - 1] / B; every other entry is the zero the
    reference leaves there."""
    hits, maxprob = np.asarray(hits), np.asarray(maxprob, dtype=np.float64)
    lead, k, n = hits.shape[:-3], hits.shape[-1], loss_fn.n_exits
    Bl = np.broadcast_to(np.asarray(B).reshape(np.shape(B) + (1,) * (len(lead) - np.ndim(B))), lead)
    acc = _fraction(hits[..., 0, -1, :], Bl[..., None], gpu_mean)                       # [..., K]: the last exit's (n_exits == 1: only the last logits count)
    out = np.zeros(lead + (len(loss_fn.metric_names),), dtype=np.float64)
    out[..., :k] = acc / n                                                    # (acc_clf.double().mean over the exit rows: one entry, n - 1 zeros)
    for i in range(k):
        out[..., k + i * (2 * n - 1)] = acc[..., i]
    out[..., -1] = maxprob[..., -1] / Bl
    return out


def _evaluate_folded(loss_fn, test_iter, model, dev, T, group=None, shard=None, device_metrics=False):
    """``_walk_folded`` with the reference's metric vector as the row: through torch (default), or from the counts of the device read-out
    (``device_metrics``); averaged over the batches per pass, then over the passes, as the reference does (train_utils.py:38,
    evaluate.py:17)."""
    if device_metrics:
        readout = _DeviceReadout(loss_fn._acc_tops, dev, lambda hits, maxprob, Bs: metric_rows_from_counts(loss_fn, hits, maxprob, Bs),
                                 len(loss_fn.metric_names))
    else:
        readout = _TorchReadout(loss_fn, dev)
    return _per_pass(_walk_folded(readout, test_iter, model, dev, T, group=group, shard=shard))


def pass_accuracy_numpy(logits, labels, tops):
    """Host restatement of bmi_pass_accuracy (``MCDEngine.pass_accuracy``), float64: ``logits`` fp32 [T, E, B, C], ``labels`` int [B],
    ``tops`` [K] -> (hits int32 [T, 2, E, K], maxprob float64 [T, E], nonfinite int).  rank(score) = #{c: score_c > score_y} +
    #{c < y: score_c == score_y} (the label loses ties to lower class indices: a stable descending sort); rank_clf[e] on the fp32 logits,
    rank_ens[e] on the float64 softmax outputs summed in exit order from exit 0; hits = #{b: rank < top}; maxprob = the rows'
    1 / sum_c exp(z_c - max) added in image order.  A row with a non-finite logit is a miss in clf[e] and ens[e' >= e], adds 0.0 and
    counts in ``nonfinite``; a label outside [0, C) is a miss everywhere."""
    lg = np.ascontiguousarray(logits, dtype=np.float32)
    T, E, B, Cd = lg.shape
    y = np.asarray(labels).astype(np.int64).reshape(B)
    tops = np.array([int(i) for i in tops], dtype=np.int64)
    labelled = (y >= 0) & (y < Cd)
    yc = np.where(labelled, y, 0)
    lower = np.arange(Cd)[None, :] < yc[:, None]                      # [B, C]: c < y
    miss = np.iinfo(np.int32).max

    def rank(score):                                                 # [T, B, C] -> [T, B]
        sy = np.take_along_axis(score, np.broadcast_to(yc[None, :, None], (T, B, 1)), axis=-1)
        return ((score > sy) | ((score == sy) & lower[None])).sum(-1)

    finite = np.isfinite(lg).all(-1)                                  # [T, E, B]
    with np.errstate(all="ignore"):
        z = lg.astype(np.float64)
        ex = np.exp(z - z.max(-1, keepdims=True))
        s = ex.sum(-1, keepdims=True)
        p = np.where(finite[..., None], ex / s, 0.0)
        m = np.where(finite, 1.0 / s[..., 0], 0.0)
        ranks = np.full((T, 2, E, B), miss, dtype=np.int64)
        ens, ens_ok = np.zeros((T, B, Cd)), np.ones((T, B), dtype=bool)
        for e in range(E):
            ens = ens + p[:, e]
            ens_ok &= finite[:, e]
            ranks[:, 0, e] = np.where(finite[:, e] & labelled[None], rank(lg[:, e]), miss)
            ranks[:, 1, e] = np.where(ens_ok & labelled[None], rank(ens), miss)
    hits = (ranks[..., None] < tops).sum(3).astype(np.int32)
    return hits, np.cumsum(m, axis=-1)[..., -1], int((~finite).sum())


def exit_metric_names(n_exits, acc_tops=(1, 5)):
    """The columns of ``evaluate_exits``' table: acc{i}_clf{e} (e major), acc{i}_ens{e}, maxprob{e}"""
    return ([f"acc{i}_clf{e}" for e in range(n_exits) for i in acc_tops] + [f"acc{i}_ens{e}" for e in range(n_exits) for i in acc_tops] +
            [f"maxprob{e}" for e in range(n_exits)])


def exit_rows_from_counts(hits, maxprob, B, gpu_mean=True):
    """``exit_metric_names``' columns from the counts of ``pass_accuracy``: every accuracy the count over B as in evaluate()'s vector
    (``_fraction``), every mean max-probability maxprob / B; ``hits`` [..., 2, E, K], ``maxprob`` [..., E] -> float64 [..., 2 E K + E]."""
    hits, maxprob = np.asarray(hits), np.asarray(maxprob, dtype=np.float64)
    lead = hits.shape[:-3]
    Bl = np.broadcast_to(np.asarray(B).reshape(np.shape(B) + (1,) * (len(lead) - np.ndim(B))), lead)[..., None]
    return np.concatenate([_fraction(hits.reshape(lead + (-1,)), Bl, gpu_mean), maxprob / Bl], axis=-1)


def evaluate_exits(test_iter, model, gpu, mc_dropout_passes, acc_tops=(1, 5), shard=None, group=None):
    """Top-k accuracy of EVERY exit and EVERY exit ensemble, and every exit's mean max-probability, per stochastic pass — what the
    reference's ``_MultiExitAccuracy`` meant to log and its row-0 overwrite loses (SA/train/loss/base_classes.py:45-48), with the standard
    deviation over the passes that SA/train/evaluate.py:18 computes and drops.  The walk is evaluate()'s folded one (same Masksembles
    counters, ``model.advance``, engine choice and sharding over the ranks of a process group), the read-out ``MCDEngine.pass_accuracy``.
    Averaged over the batches per pass, then over the passes (the order of ``validate_model_acc`` / ``evaluate``).  Returns a dict:
    ``acc_clf`` / ``acc_ens`` [E, K] (row e of ``acc_ens``: the summed softmax of exits 0..e; ``acc_ens[0] == acc_clf[0]``), ``maxprob`` [E],
    ``acc_clf_std`` / ``acc_ens_std`` / ``maxprob_std`` (``np.std`` over the passes), the per-pass tables ``acc_clf_passes`` /
    ``acc_ens_passes`` [T, E, K] and ``maxprob_passes`` [T, E], ``acc_tops`` and ``names`` (``exit_metric_names``: the columns of the flat
    [T, 2 E K + E] table ``per_pass``)."""
    model.eval()
    dev = get_device(gpu)
    if not (hasattr(model, "forward_samples_ok") and hasattr(test_iter, "__len__") and len(test_iter) > 0 and dev.type == "cuda"):
        raise ValueError("evaluate_exits needs one of the package's models on a GPU and a loader with a length")
    from ..engine import model_exits
    T, E, K = int(mc_dropout_passes), model_exits(model), len(acc_tops)
    readout = _DeviceReadout(acc_tops, dev, exit_rows_from_counts, 2 * E * K + E)
    per_pass = _per_pass(_walk_folded(readout, test_iter, model, dev, T, group=group, shard=shard))       # [T, 2 E K + E]
    tables = {"acc_clf": per_pass[:, :E * K].reshape(T, E, K), "acc_ens": per_pass[:, E * K:2 * E * K].reshape(T, E, K),
              "maxprob": per_pass[:, 2 * E * K:]}
    out = {"acc_tops": tuple(int(i) for i in acc_tops), "names": exit_metric_names(E, acc_tops), "per_pass": per_pass}
    for name, tab in tables.items():
        out[name], out[name + "_std"], out[name + "_passes"] = np.average(tab, axis=0), np.std(tab, axis=0), tab
    return out


def evaluate(loss_fn, test_iter, model, gpu, experiment_id, mc_dropout_passes, create_log=True, fold=True, shard=None, group=None,
             device_metrics=False):
    """SA/train/evaluate.py:8-22.  ``fold`` (default): the T outer passes are folded per batch (``_evaluate_folded``) when the model is one
    of the package's mirrors, the loss a MultiExitAccuracy and the loader has a length; ``fold=False`` keeps the reference's loop order
    (T walks over the loader, one ``model(X)`` per batch: 25 launches per call, host-bound — 11x slower, tools/loop_bench.py).
    ``shard`` / ``group``: the folded route partitions the T passes over the ranks of an initialised ``torch.distributed`` (see
    ``_evaluate_folded``); every rank returns the same vector, rank 0 writes the log.  ``device_metrics=True`` (folded route only): the
    metric arithmetic of a batch is ONE ``MCDEngine.pass_accuracy`` call behind its engine pass — integer hit counts and a float64
    max-probability sum, no per-sample logits beyond one engine buffer — and the vector is assembled on the host from the counts: the same
    accuracy entries bit for bit, avg_maxprob in float64 instead of torch's fp32 softmax and mean (a few 1e-7 apart)."""
    model.eval()
    dev = get_device(gpu)
    foldable = (fold and hasattr(model, "forward_samples_ok") and hasattr(loss_fn, "_metrics_passes") and hasattr(test_iter, "__len__")
                and len(test_iter) > 0 and dev.type == "cuda")
    rank = 0
    if foldable:
        from ..sharding import _rank_world
        rank = 0 if shard is False else _rank_world(group)[0]
        per_pass = _evaluate_folded(loss_fn, test_iter, model, dev, mc_dropout_passes, group=group, shard=shard, device_metrics=device_metrics)
    elif device_metrics:
        raise ValueError("device_metrics=True needs the folded route: one of the package's models on a GPU, a MultiExitAccuracy, a loader with a length")
    else:
        per_pass = np.array([validate_model_acc(loss_fn, model, test_iter, gpu) for _ in range(mc_dropout_passes)])
    averaged = list(np.average(per_pass, axis=0))
    if create_log and rank == 0:
        with open(f"log_{experiment_id}.txt", "w") as f:
            f.write(str([(n, f"{v:>8.4f}") for n, v in zip(loss_fn.metric_names, averaged)]))
    return averaged
