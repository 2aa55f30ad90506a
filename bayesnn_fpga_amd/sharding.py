"""Multi-GPU: shard the T Monte-Carlo samples (or Masksembles mask indices) over ranks.

One process per GPU (``torch.distributed``, backend "nccl" = RCCL over xGMI).  Samples are
independent given (seed, site, t) — the Philox counter carries t — so rank g runs
t in [lo_g, hi_g) on the same batch with the same seed, and the ONLY exchange is one all-reduce
(sum) of the float64 moment buffer [3, E, B, C] per batch (KBs: latency-bound, never link-bound;
SURVEY.md §8.5).  The deterministic prefix is recomputed per rank (cheaper than broadcasting it).  With fewer samples than
ranks the batch is partitioned by IMAGES instead (``partition`` / ``accumulate_partitioned``): no rank idles.
The reference has no counterpart: it is single-device (SA/train/train_utils.py:10-11).
"""
import torch


def shard_range(total, rank, world):
    """Contiguous, balanced split of range(total): the first ``total % world`` ranks get one extra."""
    if world < 1 or not (0 <= rank < world):
        raise ValueError(f"bad rank/world {rank}/{world}")
    base, extra = divmod(int(total), world)
    lo = rank * base + min(rank, extra)
    return lo, lo + base + (1 if rank < extra else 0)


def accumulate_sharded(accumulate_fn, S, T, group=None, t_begin=0):
    """Runs this rank's t-shard through ``accumulate_fn(S, t_lo, t_count)`` (which ADDS into the
    moment buffer ``S``) and sums the buffers over the group.  Works for any backend: the GPU path
    passes ``MCDEngine.accumulate`` and a RCCL group; the CPU tests pass a gloo group."""
    import torch.distributed as dist
    if dist.is_available() and dist.is_initialized():
        rank, world = dist.get_rank(group), dist.get_world_size(group)
    else:
        rank, world = 0, 1
    lo, hi = shard_range(T, rank, world)
    if hi > lo:
        accumulate_fn(S, t_begin + lo, hi - lo)
    if world > 1:
        dist.all_reduce(S, op=dist.ReduceOp.SUM, group=group)
    return S


def partition(T, B, rank, world, kind=None):
    """What rank ``rank`` of ``world`` runs of a batch of B images x T Monte-Carlo samples: ``("samples", lo, hi)`` — the
    sample range [lo, hi) on all images — while there are more samples than ranks, else ``("images", lo, hi)`` —
    ALL T samples on images [lo, hi): the fallback of SURVEY.md §8.5 ("partition by images, pure DP") for T < G, where a
    sample split would leave ranks idle (T = 4 on 8 GPUs: half of them) and every rank would still recompute the whole
    once-per-batch prefix.  Either way the shares are disjoint and their moment buffers add up to the one-rank result.
    T == world (config 4: one Masksembles mask per GPU) also goes by images: measured on one MI355X, rank 0's share of eight as
    32 images x 8 samples takes 0.61 ms per batch against 0.77 ms as 250 images x 1 sample (tools/share_bench.py,
    profiles/r04_share_config4.txt: the prefix runs on 32 images instead of 250 and a head launch's 32-sample groups are full) —
    every GPU then applies all M masks to its images instead of one mask to all images; the reduce is the same one all-reduce.
    (T > world keeps the sample split the configs are written with — "T=512 sharded 64/GPU" — although the image split measured
    6 % faster there too: 3.00 vs 3.18 ms for T = 100 over eight ranks; ``kind`` / ``bench.py --partition`` force either.)"""
    if kind not in (None, "samples", "images"):
        raise ValueError(f"kind must be 'samples' or 'images', got {kind!r}")
    if kind is None:
        kind = "samples" if world == 1 or ((T > world or B < world) and T >= world) else "images"
    return (kind,) + (shard_range(T, rank, world) if kind == "samples" else shard_range(B, rank, world))


def _rank_world(group=None):
    import torch.distributed as dist
    if dist.is_available() and dist.is_initialized():
        return dist.get_rank(group), dist.get_world_size(group)
    return 0, 1


def share_kind(engine, T, B, world, kind=None):
    """``partition``'s choice for this engine: with ``kind=None`` an image split that some rank's kernels cannot take (a share that
    does not start on a whole Philox call of every site, ``bmi_image_offset_ok``: e.g. B = 250 over 8 ranks with a 32-channel
    channel-wise site) falls back to the sample split — host-only and the same answer on every rank, so the choice stays
    collective-safe.  An explicit ``kind="images"`` that cannot be taken raises on every rank together."""
    chosen = partition(T, B, 0, world, kind)[0]
    if chosen != "images":
        return chosen
    # every rank checks EVERY rank's image offset: a partition is accepted or refused by the whole group before anyone launches,
    # instead of one rank raising while the others wait in the all-reduce
    bad = [r for r in range(world) if not engine.image_offset_ok(shard_range(B, r, world)[0])]
    if not bad:
        return "images"
    if kind is None:
        return "samples"
    raise ValueError(f"image partition of a batch of {B} over {world} ranks: the shares of ranks {bad} do not start on a "
                     "whole Philox call of every site (bmi_image_offset_ok)")


def accumulate_share(engine, x, S, T, seed=0, cnt0=0, rank=0, world=1, kind=None, H=None):
    """Rank ``rank``'s share of batch ``x`` x T samples ADDED into the moment buffer ``S`` [3, E, B, C]; NO collective (what a
    hipGraph of a rank's step captures: ``BatchesInFlight.predict_graphed``).  ``partition`` decides (``share_kind``): by samples
    while T > world size; by images when T <= world — the rank runs ``engine.accumulate(x[lo:hi], ..., image_offset=lo)``, masks
    drawn at the images' indices in the whole batch (bmi_forward_mcd_images), into its rows of S (the other ranks' rows stay zero
    until the all-reduce) — unless some rank's share cannot start where the split puts it: then by samples after all
    (``kind=None``), or a ValueError on every rank (explicit ``kind="images"``).  Nothing is allocated here: the share's
    [3, E, hi - lo, C] staging buffer belongs to the engine.  ``H``: the entropy sums [E, B] beside S (``new_uncertainty_sums``), added
    into as well (``engine.accumulate_uncertainty``); returns (S, H) then."""
    B = x.shape[0]
    kind = share_kind(engine, T, B, world, kind)
    _, lo, hi = partition(T, B, rank, world, kind)
    out = S if H is None else (S, H)

    def run(x, S, H, t_begin, t_count, image_offset):
        if H is None:
            engine.accumulate(x, S, t_begin, t_count, seed, cnt0, image_offset=image_offset)
        else:
            engine.accumulate_uncertainty(x, S, H, t_begin, t_count, seed, cnt0, image_offset=image_offset)

    if hi <= lo:
        return out
    if kind == "samples":
        run(x, S, H, lo, hi - lo, 0)
        return out
    cache = engine.__dict__.setdefault("_share_parts", {})
    key = (H is not None, S.shape[1], hi - lo, S.shape[3])
    part = cache.get(key)
    if part is None:                # first call of this share shape only
        part = cache[key] = (S.new_zeros(3, S.shape[1], hi - lo, S.shape[3]), None) if H is None else \
            new_uncertainty_sums(S.shape[1], hi - lo, S.shape[3], S.device)
    else:
        (part[0] if H is None else _packed(*part)).zero_()
    run(x[lo:hi], *part, 0, T, lo)
    S[:, :, lo:hi].add_(part[0])
    if H is not None:
        H[:, lo:hi].add_(part[1])
    return out


def accumulate_partitioned(engine, x, S, T, seed=0, cnt0=0, group=None, kind=None, always_reduce=False, H=None):
    """This rank's share of batch ``x`` x T samples ADDED into the moment buffer ``S`` [3, E, B, C] (``accumulate_share``), then ONE
    all-reduce (sum) over the group.  ``always_reduce``: issue the collective in a group of ONE rank too (a sum over one rank: the same
    bits) — how a 1-GPU box exercises RCCL on exactly the streams and buffers the N-GPU path uses (bench.py's ``allreduce_us_1rank``).
    ``H``: the entropy sums beside S, views of one buffer (``new_uncertainty_sums``): that buffer is what the all-reduce sums; returns
    (S, H) then."""
    import torch.distributed as dist
    rank, world = _rank_world(group)
    buf = S if H is None else _packed(S, H)
    out = accumulate_share(engine, x, S, T, seed, cnt0, rank, world, kind, H=H)
    if world > 1 or (always_reduce and dist.is_available() and dist.is_initialized()):
        dist.all_reduce(buf, op=dist.ReduceOp.SUM, group=group)
    return out


def predict_sharded(engine, x, T, seed=0, cnt0=0, group=None):
    """mean / var / logit_mean of T samples with the work partitioned over the process group (by samples, or by images
    when there are fewer samples than ranks)."""
    S = engine.new_moments(x.shape[0])
    accumulate_partitioned(engine, x, S, T, seed, cnt0, group)
    return engine.finalize(S, T)


def new_uncertainty_sums(n_exits, batch, out_dim, device=None):
    """S [3, E, B, C] and H [E, B], zeroed float64 views of ONE allocation (``S._base``: what ``accumulate_partitioned(..., H=H)``
    all-reduces)."""
    n = 3 * n_exits * batch * out_dim
    buf = torch.zeros(n + n_exits * batch, dtype=torch.float64, device=device)
    return buf[:n].view(3, n_exits, batch, out_dim), buf[n:].view(n_exits, batch)


def _packed(S, H):
    buf = S._base
    if buf is None or H._base is not buf or buf.numel() != S.numel() + H.numel() or not buf.is_contiguous():
        raise ValueError("S and H must be the two views of one buffer (new_uncertainty_sums)")
    return buf


def accumulate_partitioned_uncertainty(engine, x, S, H, T, seed=0, cnt0=0, group=None, kind=None):
    """``accumulate_partitioned`` with the entropy sums H [E, B] beside S."""
    return accumulate_partitioned(engine, x, S, T, seed, cnt0, group, kind, H=H)


def predict_sharded_uncertainty(engine, x, T, seed=0, cnt0=0, group=None):
    """``predict_sharded`` with the uncertainty decomposition (``MCDEngine.finalize_uncertainty``)."""
    S, H = engine.new_uncertainty_sums(x.shape[0])
    accumulate_partitioned(engine, x, S, T, seed, cnt0, group, H=H)
    return engine.finalize_uncertainty(S, H, T)
