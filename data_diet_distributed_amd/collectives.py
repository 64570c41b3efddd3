"""The shard layout and the collectives of a scoring job: batch-aligned contiguous shards, and
an all-gather / all-reduce that every caller shares.  On GPU with the "nccl" backend these are
RCCL over xGMI; under gloo (`_via_host`) device tensors are staged through host memory."""
from __future__ import annotations

import torch
import torch.distributed as dist


def _world(group=None):
    if dist.is_available() and dist.is_initialized():
        return dist.get_world_size(group), dist.get_rank(group)
    return 1, 0


def world_of(group=None) -> int:
    return _world(group)[0]


def shard_bounds(n: int, batch_size: int, world: int, rank: int):
    """Contiguous, batch-aligned shard [lo, hi) of rank `rank`:
    rank r gets batches floor(r*nb/W) .. floor((r+1)*nb/W)-1 of nb = ceil(n/B)."""
    if world <= 0 or not 0 <= rank < world:
        raise ValueError("bad rank/world")
    nb = -(-n // batch_size)
    b_lo = (rank * nb) // world
    b_hi = ((rank + 1) * nb) // world
    return min(n, b_lo * batch_size), min(n, b_hi * batch_size)


def all_shards(n: int, batch_size: int, world: int):
    return [shard_bounds(n, batch_size, world, r) for r in range(world)]


def _via_host(group) -> bool:
    """gloo (CPU tests; ranks sharing one GPU, where RCCL refuses a second communicator on the
    device): device tensors are staged through host memory."""
    return dist.get_backend(group) == "gloo"


def _all_gather_same(t: torch.Tensor, group=None):
    """All-gather a same-shape tensor from every rank -> list in rank order."""
    world = dist.get_world_size(group)
    if _via_host(group):
        host = t.cpu()
        parts = [torch.empty_like(host) for _ in range(world)]
        dist.all_gather(parts, host, group=group)
        return [p.to(t.device) for p in parts]
    flat = torch.empty((world,) + tuple(t.shape), dtype=t.dtype, device=t.device)
    dist.all_gather_into_tensor(flat, t.contiguous(), group=group)
    return list(flat.unbind(0))


def _all_reduce_sum(t: torch.Tensor, group=None):
    """In-place sum over ranks."""
    if _via_host(group):
        host = t.cpu()
        dist.all_reduce(host, group=group)
        t.copy_(host)
    else:
        dist.all_reduce(t, group=group)


def shard_lengths(n: int, group=None):
    """(rows per rank in rank order, this rank): one small all-gather, once per scoring call."""
    world, rank = _world(group)
    if world == 1:
        return [int(n)], 0
    dev = "cpu" if _via_host(group) else torch.device("cuda", torch.cuda.current_device())
    parts = _all_gather_same(torch.tensor([int(n)], dtype=torch.int64, device=dev), group)
    return [int(p.item()) for p in parts], rank


def gather_padded(t: torch.Tensor, lengths, group=None) -> torch.Tensor:
    """Every rank's rows [n_r, ...] in rank order -> [sum n_r, ...] on every rank, one
    all-gather: each rank contributes its rows padded to the longest (`lengths`: rows per rank,
    known to all), and each part is cut back to its length."""
    buf = torch.zeros((max(lengths),) + tuple(t.shape[1:]), dtype=t.dtype, device=t.device)
    buf[:t.shape[0]] = t
    return torch.cat([p[:m] for p, m in zip(_all_gather_same(buf, group), lengths)])


def gather_rows(t: torch.Tensor, lengths, group=None) -> torch.Tensor:
    """gather_padded with shard_lengths' `lengths`; with one rank, `t` itself, no collective."""
    return t if len(lengths) == 1 else gather_padded(t, lengths, group)


def gather_scores(local: torch.Tensor, n: int, batch_size: int, group=None) -> torch.Tensor:
    """All-gather per-rank score shards into the full [n] vector (every rank gets it): one
    collective; the indices are implicit in the shard bounds."""
    if not dist.is_available() or not dist.is_initialized():
        if local.numel() != n:
            raise ValueError("single-process gather needs the whole score vector")
        return local
    bounds = all_shards(n, batch_size, dist.get_world_size(group))
    return gather_padded(local, [hi - lo for lo, hi in bounds], group)
