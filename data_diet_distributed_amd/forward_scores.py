"""The consumers of the EL2N pass's train-BN forward: LogitScores (el2n + LOGIT_METHODS, from
each launch's logits), ProtoScore, KMeansScore, NNScore, KNNScore, KDEScore and MahaScore (from
the checkpoint's pooled feature rows, over every rank), and ForwardScores, which holds the
requested ones for one score_shard call.

The pass hands every launch's logits to `consume` and, when `features` is not None, writes the
launch's feature rows there; after a checkpoint's last chunk it calls `end_checkpoint`.  Every
rank issues its collectives in the same order: the counts all-reduce (proto) and the lengths and
labels all-gathers (nn, the knn scores, the density scores and maha: one of each, shared,
GatheredRows; kmeans alone takes the lengths only) at construction, then per checkpoint the
proto all-reduce, the kmeans all-reduces (the seed rows, then one per Lloyd iteration) and last
the one all-gather of the feature rows that nn, the knn scores, the density scores and maha
share.
"""
from __future__ import annotations

import math
from typing import Dict, List, Optional

import torch

from . import _capi
from .collectives import _all_reduce_sum, gather_rows, shard_lengths, world_of
from .methods import DENSITY_METHODS, KNN_METHODS, LOGIT_FAMILY


def check_class_sizes(largest: int):
    """The proto score's fixed-point class sums (|q| < 2^39 per element, int64) hold fewer than
    2^24 members per class: reject a larger class."""
    if largest >= _capi.PROTO_MAX_CLASS:
        raise ValueError(f"proto: a class of {largest} members; the exact int64 feature sums "
                         f"hold fewer than {_capi.PROTO_MAX_CLASS} (2^24) per class")


def check_no_singleton_class(counts, what="nn"):
    """The nn score of a class's only member would be infinite (no other row of its class), and
    so would its kde_post (`what` names the score): reject a dataset with such a class, naming
    it.  counts: members per class over the whole dataset (an empty class is fine)."""
    for c, m in enumerate(counts):
        if int(m) == 1:
            raise ValueError(f"{what}: class {c} has exactly one member in the whole dataset; its "
                             f"nearest same-class neighbour does not exist (score +inf)")


def _check_width(name: str, D: int):
    if D > _capi.PROTO_MAX_D:
        raise ValueError(f"{name}: feature width {D} above {_capi.PROTO_MAX_D}")


def class_grouping(labels: torch.Tensor, num_classes: int):
    """(order, offsets, counts, bad) of int64 device labels [n]: the rows stable-sorted by class
    with the labels outside [0, C) last (past offsets[C]: in no class), the int64 [C + 1] class
    offsets, and dd_class_counts' outputs."""
    C = int(num_classes)
    counts, bad = _capi.class_counts(labels, C, check=False)
    key = torch.where((labels >= 0) & (labels < C), labels, torch.full_like(labels, C))
    off = torch.zeros(C + 1, dtype=torch.int64, device=labels.device)
    off[1:] = torch.cumsum(counts, 0)
    return torch.argsort(key, stable=True), off, counts, bad


def nearest_same_class(features: torch.Tensor, labels: torch.Tensor, num_classes: int,
                       operands: str = "f16x3") -> torch.Tensor:
    """fp32 [n]: each row's distance to the nearest other row of its class among `features`
    [n, D] (one dd_nn_same_class launch; a tie goes to the smaller row index).  Raises
    LabelError for a label outside [0, C) and ValueError for a class of exactly one member."""
    labels = labels.contiguous()
    order, off, counts, bad = class_grouping(labels, num_classes)
    host = torch.cat([counts, bad.to(torch.int64)]).tolist()  # the one read of the counts
    if host[-1]:
        raise _capi.LabelError(f"nn: {host[-1]} label(s) outside [0, {int(num_classes)})")
    check_no_singleton_class(host[:-1])
    rows = features.index_select(0, order)
    dist_sorted = torch.empty(rows.shape[0], dtype=torch.float32, device=rows.device)
    _capi.nn_same_class(rows, order, off, rows, order, off, operands=operands, dist=dist_sorted)
    return torch.empty_like(dist_sorted).index_copy_(0, order, dist_sorted)


def check_knn_size(N: int, k: int):
    """Every row of the knn scores needs k other rows: reject a dataset of N <= k rows."""
    if N <= k:
        raise ValueError(f"knn_k={k} needs more than {k} examples in the whole dataset (got "
                         f"{N}): a row would have fewer than knn_k neighbours (score +inf)")


def nearest_k(features: torch.Tensor, labels: torch.Tensor, num_classes: int, k: int,
              operands: str = "f16x3"):
    """(knn fp32 [n], knn_disagree fp32 [n]): each row's mean distance to its k nearest other
    rows of `features` [n, D], any class, and the share of them with another label (one dd_knn
    launch; a tie goes to the smaller row index).  Raises LabelError for a label outside [0, C)
    and ValueError for n <= k."""
    labels = labels.contiguous()
    _capi.class_counts(labels, num_classes, check=True)
    n = features.shape[0]
    check_knn_size(n, k)
    ids = torch.arange(n, dtype=torch.int64, device=features.device)
    mean = torch.empty(n, dtype=torch.float32, device=features.device)
    share = torch.empty_like(mean)
    _capi.knn(features, ids, features, ids, k, q_label=labels, c_label=labels, operands=operands,
              mean_dist=mean, disagree=share)
    return mean, share


KDE_SCALE_ROWS = 1 << 16  # rows per float64 block of kde_scale (fixed: the order is part of s)


def kde_scale(rows: torch.Tensor) -> float:
    """s of the density scores: the mean squared distance over all ordered pairs of distinct rows
    of `rows` [N, D], s = 2 N / (N - 1) (mean ||f||^2 - ||mean f||^2), in float64 over fixed
    blocks of rows in the order given (a function of the rows and their order alone; one read
    back).  A row with a non-finite element, which the kernel ignores as a candidate, is left
    out, N counting the others.  Raises ValueError where no positive scale exists (fewer than two
    finite rows, or all of them equal)."""
    D = rows.shape[1]
    acc = torch.zeros(D + 2, dtype=torch.float64, device=rows.device)  # sum f, sum ||f||^2, N
    for r0 in range(0, rows.shape[0], KDE_SCALE_ROWS):
        x = rows[r0:r0 + KDE_SCALE_ROWS].double()
        ok = torch.isfinite(x).all(dim=1)
        x = torch.where(ok[:, None], x, torch.zeros_like(x))
        acc[:D] += x.sum(dim=0)
        acc[D] += (x * x).sum()
        acc[D + 1] += ok.sum()
    host = acc.cpu()
    N = float(host[D + 1])
    if N < 2:
        raise ValueError(f"kde: needs at least two finite feature rows (got {int(N)})")
    s = 2.0 * N / (N - 1.0) * (float(host[D]) / N - float((host[:D] / N).square().sum()))
    if not 0.0 < s < float("inf"):
        raise ValueError(f"kde: the feature rows have no positive mean squared distance (s={s})")
    return s


def density(features: torch.Tensor, labels: torch.Tensor, num_classes: int, bandwidth: float,
            operands: str = "f16x3"):
    """(kde fp32 [n], kde_post fp32 [n]): each row's negative log kernel density among the other
    rows of `features` [n, D] and the negative log Parzen posterior of its own label, the weights
    exp(-d^2 / (bandwidth s)) with s = kde_scale(features) (one dd_kde launch).  Raises LabelError
    for a label outside [0, C) and ValueError for a class of exactly one member."""
    from .methods import check_bandwidth
    bandwidth = check_bandwidth(bandwidth)
    labels = labels.contiguous()
    counts, _ = _capi.class_counts(labels, num_classes, check=True)
    check_no_singleton_class(counts.tolist(), "kde_post")
    n = features.shape[0]
    ids = torch.arange(n, dtype=torch.int64, device=features.device)
    nll = torch.empty(n, dtype=torch.float32, device=features.device)
    post = torch.empty_like(nll)
    _capi.kde(features, ids, features, ids, 1.0 / (bandwidth * kde_scale(features)),
              q_label=labels, c_label=labels, operands=operands, nll=nll, post=post)
    return nll.add_(math.log(max(n - 1, 1))), post


def kmeans_seed_rows(N: int, k: int) -> List[int]:
    """The dataset rows the k centroids start from: s_j = floor((2 j + 1) N / (2 k)), evenly
    spaced, distinct for N >= k, and a function of N and k alone."""
    return [((2 * j + 1) * N) // (2 * k) for j in range(k)]


def check_kmeans_size(N: int, k: int):
    """k-means needs a seed row per cluster, and its fixed-point sums (|q| < 2^39 per element,
    int64) hold fewer than 2^24 rows in one cluster: reject a dataset outside k <= N < 2^24."""
    if N < k:
        raise ValueError(f"kmeans_k={k} needs at least {k} examples in the whole dataset (got "
                         f"{N}): every cluster starts from a row of its own")
    if N >= _capi.KMEANS_MAX_N:
        raise ValueError(f"kmeans: {N} examples; the exact int64 feature sums hold fewer than "
                         f"{_capi.KMEANS_MAX_N} (2^24) rows in one cluster")


def lloyd_step(features, centroids, reduce, workspace, operands, repack, group=None, world=1):
    """One Lloyd update of `centroids` [k, D] in place from this rank's rows `features`: the
    int64 buffer `reduce` [k D + k + 1] (the sums, the counts, the unrepresentable rows) is
    cleared, filled by one dd_kmeans_assign launch, summed over `group`'s `world` ranks (an exact
    integer all-reduce) and turned into the centroids.  Returns the workspace."""
    k, D = centroids.shape
    reduce.zero_()
    workspace, _ = _capi.kmeans_assign(
        features, centroids, operands=operands, repack_rows=repack,
        sums=reduce[:k * D].view(k, D), counts=reduce[k * D:k * D + k], bad=reduce[k * D + k:],
        workspace=workspace)
    if world > 1:
        _all_reduce_sum(reduce, group)
    _capi.kmeans_centroids(reduce[:k * D].view(k, D), reduce[k * D:k * D + k], centroids)
    return workspace


def kmeans(features: torch.Tensor, k: int, iters: int, operands: str = "f16x3"):
    """(centroids fp32 [k, D], assign int32 [n], dist fp32 [n]): `iters` Lloyd updates over the rows
    of `features` [n, D] from the seed rows kmeans_seed_rows(n, k), then each row's nearest
    centroid (a tie goes to the smaller cluster id) and its distance to it (include/dd_capi.h
    dd_kmeans_assign).  Raises ValueError for n < k and, after one read of the kernel's counter,
    for a row with a NaN, an infinity or |v| >= 2^15 (its distance would be NaN)."""
    n, D = features.shape
    k, iters = int(k), int(iters)
    _check_width("kmeans", D)
    check_kmeans_size(n, k)
    dev = features.device
    seeds = torch.tensor(kmeans_seed_rows(n, k), dtype=torch.int64).to(dev)
    centroids = features.index_select(0, seeds).contiguous()
    reduce = torch.empty(k * D + k + 1, dtype=torch.int64, device=dev)
    ws = None
    for it in range(iters):
        ws = lloyd_step(features, centroids, reduce, ws, operands, it == 0)
    assign = torch.empty(n, dtype=torch.int32, device=dev)
    dist = torch.empty(n, dtype=torch.float32, device=dev)
    _, bad = _capi.kmeans_assign(features, centroids, operands=operands, repack_rows=ws is None,
                                 assign=assign, dist=dist, workspace=ws)
    if int(bad.item()):
        raise ValueError(f"kmeans: {int(bad.item())} feature row(s) with a NaN, an infinite or an "
                         f"|v| >= 2^15 element: their distance is undefined")
    return centroids, assign, dist


def class_means(features: torch.Tensor, labels: torch.Tensor, counts: torch.Tensor, order=None):
    """(mean fp32 [C, D], bad_feat int32 [C]) of `features` [N, D], every row of the dataset:
    proto's class means (dd_class_feature_sums -> dd_class_centroids: the exact fixed-point sums,
    the same rounding) and its per-class counts of rows with a NaN, an infinite or an
    |v| >= 2^15 element."""
    C, D = counts.numel(), features.shape[1]
    sums = torch.zeros((C, D), dtype=torch.int64, device=features.device)
    bad_feat = torch.zeros(C, dtype=torch.int32, device=features.device)
    _capi.class_feature_sums(features, labels, sums, bad_feat, order=order)
    return _capi.class_centroids(sums, counts, bad_feat), bad_feat


def maha_whitener(S: torch.Tensor, N: int, shrink: float) -> torch.Tensor:
    """W fp32 [D, D] on S's device, lower triangular with W Sigma W^T = I for Sigma = S / N +
    shrink (trace(S / N) / D) I: the float64 algebra between dd_maha_scatter and dd_maha_dist, on
    the host (one D x D copy each way; not a hot path).  Raises ValueError if Sigma has no
    Cholesky factor."""
    sigma = S.detach().to("cpu", torch.float64) / float(N)
    D = sigma.shape[0]
    sigma.diagonal().add_(float(shrink) * float(sigma.diagonal().sum()) / D)
    L, info = torch.linalg.cholesky_ex(sigma)
    if int(info) or not bool(torch.isfinite(L).all()):
        raise ValueError(f"maha: the covariance is not positive definite at maha_shrink={shrink} "
                         f"(N={N} rows, D={D}): raise maha_shrink")
    W = torch.linalg.solve_triangular(L, torch.eye(D, dtype=torch.float64), upper=False)
    return torch.tril(W).to(torch.float32).to(S.device)


def check_maha_rows(bad_feat: torch.Tensor, nonfinite: torch.Tensor):
    """One read of the two counters: reject feature rows the class means or the scatter cannot
    take, naming how many."""
    bad, nf = int(bad_feat.sum().item()), int(nonfinite.item())
    if bad or nf:
        raise ValueError(f"maha: {max(bad, nf)} feature row(s) with a NaN, an infinite or an "
                         f"|v| >= 2^15 element ({nf} non-finite): the covariance is undefined")


def maha(rows: torch.Tensor, labels: torch.Tensor, num_classes: int, shrink: float = 0.01,
         operands: str = "f16x3") -> torch.Tensor:
    """fp32 [n]: each row's Mahalanobis distance to its class mean under the tied within-class
    covariance of `rows` [n, D] (include/dd_capi.h dd_maha_scatter), shrunk by `shrink` towards
    its mean eigenvalue; exactly 0 for the only row of a class.  Raises LabelError for a label
    outside [0, C) and ValueError for a row with a NaN, an infinite or an |v| >= 2^15 element or a
    covariance without a Cholesky factor (maha_shrink too small)."""
    from .methods import check_shrink
    shrink = check_shrink(shrink)
    _check_width("maha", rows.shape[1])
    labels = labels.contiguous()
    counts, _ = _capi.class_counts(labels, num_classes, check=True)
    check_class_sizes(int(counts.max().item()))
    mean, bad_feat = class_means(rows, labels, counts)
    S, nonfinite, ws = _capi.maha_scatter(rows, labels, counts, mean, operands=operands)
    check_maha_rows(bad_feat, nonfinite)
    W = maha_whitener(S, rows.shape[0], shrink)
    dist = torch.empty(rows.shape[0], dtype=torch.float32, device=rows.device)
    _capi.maha_dist(rows, labels, counts, mean, W, operands=operands, dist=dist, workspace=ws)
    return dist


def ensemble_mean(acc: torch.Tensor, K: int) -> torch.Tensor:
    out = torch.empty_like(acc)
    _capi.ensemble_finalize(acc, K, out)
    return out


def _tensors(obj) -> List[torch.Tensor]:
    """Every device buffer among an object's attributes, and in those that are dicts."""
    vals = [v for a in vars(obj).values() for v in (a.values() if isinstance(a, dict) else [a])]
    return [t for t in vals if isinstance(t, torch.Tensor)]


class LogitScores:
    """The accumulators [n] of the requested members of LOGIT_FAMILY.  `acc["variability"]` is
    Welford's M2 of wrong_mass over the checkpoints and `var_mean` its mean."""

    def __init__(self, methods, n: int, device):
        self.acc = {m: torch.zeros(n, dtype=torch.float32, device=device) for m in methods}
        self.var_mean = (torch.zeros_like(self.acc["variability"])
                         if "variability" in self.acc else None)

    def consume(self, ckpt_index: int, logits, labels, r0: int, r1: int, counter):
        """One launch's logits of checkpoint `ckpt_index` (0-based) into rows [r0, r1): dd_el2n
        runs only if el2n is requested, and one dd_logit_scores launch serves all the others.
        `counter` (the pass's label counter, or None) goes to whichever runs first, so a row is
        counted once."""
        acc = self.acc
        if "el2n" in acc:
            _capi.el2n(logits, labels, accum=acc["el2n"][r0:r1], bad_labels=counter)
            counter = None
        kw = {m: acc[m][r0:r1] for m in _capi.LOGIT_STATS if m in acc}
        if self.var_mean is not None:
            kw.update(var_mean=self.var_mean[r0:r1], var_m2=acc["variability"][r0:r1],
                      k=1 + ckpt_index)
        if kw:
            _capi.logit_scores(logits, labels, bad_labels=counter, **kw)

    def finalize(self, K: int) -> Dict[str, torch.Tensor]:
        out = {m: ensemble_mean(a, K) for m, a in self.acc.items() if m != "variability"}
        if self.var_mean is not None:
            out["variability"] = torch.empty_like(self.var_mean)
            _capi.variability_finalize(self.acc["variability"], K, out["variability"])
        return out


class ProtoScore:
    """The per-call state of the proto score for the shard's `labels` [n], allocated once and
    reused by every checkpoint: the rows' order sorted by label, the class counts over every
    rank (dd_class_counts + one all-reduce: labels do not change across checkpoints; `bad` is
    this shard's count of labels outside [0, C)), and the int64 buffer [C D + C] that is
    all-reduced per checkpoint, whose first C D elements are the fixed-point `sums`."""

    def __init__(self, labels: torch.Tensor, linear, group, batch_size: int):
        n, dev = labels.numel(), labels.device
        C, D = linear.out_features, linear.in_features
        _check_width("proto", D)
        self.group, self.world = group, world_of(group)
        self.labels = labels.contiguous()
        self.counts, self.bad = _capi.class_counts(self.labels, C, check=False)
        if self.world > 1:
            _all_reduce_sum(self.counts, group)
        # the fixed-point sums hold fewer than 2^24 members per class; the shards are balanced
        # to within a batch, so the counts are read back only where the set could be that large
        if self.world * (n + batch_size) >= _capi.PROTO_MAX_CLASS:
            check_class_sizes(int(self.counts.max().item()))
        self.order = torch.argsort(self.labels, stable=True)
        self.reduce = torch.zeros(C * D + C, dtype=torch.int64, device=dev)
        self.sums = self.reduce[:C * D].view(C, D)
        self.bad_feat = torch.zeros(C, dtype=torch.int32, device=dev)
        self.centroids = torch.empty((C, D), dtype=torch.float32, device=dev)
        self.accum = torch.zeros(n, dtype=torch.float32, device=dev)

    def end_checkpoint(self, features: torch.Tensor):
        """On the current stream, after every chunk of the checkpoint has written its rows of
        `features`: one sums launch over the shard, one all-reduce, the centroids, one distance
        launch."""
        nsum = self.sums.numel()
        self.reduce.zero_()
        self.bad_feat.zero_()
        _capi.class_feature_sums(features, self.labels, self.sums, self.bad_feat,
                                 order=self.order)
        if self.world > 1:
            # one int64 buffer: the sums, then the per-class counts of unrepresentable rows
            self.reduce[nsum:].copy_(self.bad_feat)
            _all_reduce_sum(self.reduce, self.group)
            self.bad_feat.copy_(self.reduce[nsum:])
        _capi.class_centroids(self.sums, self.counts, self.bad_feat, out=self.centroids)
        _capi.proto_scores(features, self.labels, self.centroids, accum=self.accum)

    def finalize(self, K: int) -> Dict[str, torch.Tensor]:
        return {"proto": ensemble_mean(self.accum, K)}


class KMeansScore:
    """The per-call state of the kmeans score for the shard's `labels` [n] (read only for `bad`,
    this shard's count of labels outside [0, C): the clustering takes no labels), built once and
    reused by every checkpoint: the seed rows this rank owns among kmeans_seed_rows of the whole
    dataset (`lengths` / `rank`: the shard lengths, GatheredRows' where nn or the knn scores hold
    them), the centroids [k, D], the int64 buffer [k D + k + 1] that is all-reduced per Lloyd
    iteration (sums, counts, unrepresentable rows), the accumulator and the kernel's workspace
    (4 (n + k) pad16(D) bytes).  A dataset outside k <= N < 2^24 is rejected."""

    def __init__(self, labels: torch.Tensor, linear, group, lengths, rank: int, operands: str,
                 k: int, iters: int):
        n, dev = labels.numel(), labels.device
        C, D = linear.out_features, linear.in_features
        _check_width("kmeans", D)
        self.k, self.iters = int(k) or C, int(iters)  # (kmeans_k = 0: the class count)
        N, offset = sum(lengths), sum(lengths[:rank])
        check_kmeans_size(N, self.k)
        self.group, self.world, self.operands = group, len(lengths), operands
        _, self.bad = _capi.class_counts(labels.contiguous(), C, check=False)
        mine = [(j, s - offset) for j, s in enumerate(kmeans_seed_rows(N, self.k))
                if offset <= s < offset + n]
        self.seed_j, self.seed_row = (torch.tensor([m[i] for m in mine], dtype=torch.int64).to(dev)
                                      for i in (0, 1))
        self.centroids = torch.empty((self.k, D), dtype=torch.float32, device=dev)
        self.reduce = torch.empty(self.k * D + self.k + 1, dtype=torch.int64, device=dev)
        self.accum = torch.zeros(n, dtype=torch.float32, device=dev)
        need = _capi.kmeans_workspace_bytes(n, self.k, D, operands)
        self.workspace = torch.empty(max(need, 1), dtype=torch.uint8, device=dev)

    def end_checkpoint(self, features: torch.Tensor):
        """At the same point of a checkpoint as ProtoScore's, on the current stream, nothing read
        back: the seed rows (each rank writes those it owns into zeros; the int32 view is summed,
        so that adding zeros changes no bit), `iters` Lloyd updates (the rows' operand halves are
        made by the first), and the scoring assignment."""
        self.centroids.zero_()
        self.centroids.index_copy_(0, self.seed_j, features.index_select(0, self.seed_row))
        if self.world > 1:
            _all_reduce_sum(self.centroids.view(torch.int32), self.group)
        for it in range(self.iters):
            self.workspace = lloyd_step(features, self.centroids, self.reduce, self.workspace,
                                        self.operands, it == 0, self.group, self.world)
        _capi.kmeans_assign(features, self.centroids, operands=self.operands, repack_rows=False,
                            accum=self.accum, bad=self.reduce[-1:], workspace=self.workspace)

    def finalize(self, K: int) -> Dict[str, torch.Tensor]:
        """(`reduce[-1]` holds the last assignment's count of unrepresentable rows over every rank
        for a caller that wants to name them; the engine reads nothing back here: such a row's
        score is NaN, which ScoringEngine._validate rejects or re-scores on bf16 halves.)"""
        return {"kmeans": ensemble_mean(self.accum, K)}


class GatheredRows:
    """The shard's place among every rank's rows, shared by nn and the knn scores: the shard
    lengths and this rank's index (one all-gather), every rank's labels (one all-gather; labels
    do not change across checkpoints; `labels` itself on one rank) and, per checkpoint, `gather`:
    the one all-gather of the feature rows."""

    def __init__(self, labels: torch.Tensor, group):
        self.group = group
        self.lengths, self.rank = shard_lengths(labels.numel(), group)
        self.labels = gather_rows(labels, self.lengths, group)
        self.local = self.labels is labels  # one rank: the candidates are the queries
        self.offset = sum(self.lengths[:self.rank])

    def gather(self, features: torch.Tensor) -> torch.Tensor:
        return gather_rows(features, self.lengths, self.group)


class NNScore:
    """The per-call state of the nn score for the shard's `labels` [n], built once and reused by
    every checkpoint: from every rank's labels (`rows`) the class offsets of the whole dataset
    and of this shard (dd_class_counts; `bad` is this shard's count of labels outside [0, C)),
    the class-sorted order of the candidates (all rows) and of the queries (this rank's rows)
    with their global ids, the class-ordered row buffers, the class-ordered accumulator and the
    kernel's workspace (4 (n + N) pad16(D) bytes).
    The whole dataset's counts are read to the host once: a class of exactly one member is
    rejected by name."""

    def __init__(self, labels: torch.Tensor, linear, rows: GatheredRows, operands: str):
        n, dev = labels.numel(), labels.device
        C, D = linear.out_features, linear.in_features
        _check_width("nn", D)
        self.operands = operands
        all_labels = rows.labels
        self.q_order, self.q_off, counts, self.bad = class_grouping(labels, C)
        if rows.local:  # one rank: the candidates are the queries
            self.c_order, self.c_off, self.c = self.q_order, self.q_off, None
        else:
            self.c_order, self.c_off, counts, _ = class_grouping(all_labels.contiguous(), C)
            self.c = torch.empty((all_labels.numel(), D), dtype=torch.float32, device=dev)
        check_no_singleton_class(counts.tolist())  # the one read of the counts
        self.q_id = self.q_order + rows.offset
        self.q = torch.empty((n, D), dtype=torch.float32, device=dev)
        self.accum = torch.zeros(n, dtype=torch.float32, device=dev)
        need = _capi.nn_workspace_bytes(n, all_labels.numel(), D, operands)
        self.workspace = torch.empty(max(need, 1), dtype=torch.uint8, device=dev)

    def end_checkpoint(self, features: torch.Tensor, allf: torch.Tensor):
        """At the same point of a checkpoint as ProtoScore's, with every rank's feature rows
        `allf` (GatheredRows.gather): the rows gathered into class order, one dd_nn_same_class
        launch that accumulates in class order."""
        torch.index_select(features, 0, self.q_order, out=self.q)
        cand = self.q if self.c is None else torch.index_select(allf, 0, self.c_order,
                                                                out=self.c)
        self.workspace = _capi.nn_same_class(
            self.q, self.q_id, self.q_off, cand, self.c_order, self.c_off,
            operands=self.operands, accum=self.accum, workspace=self.workspace)

    def finalize(self, K: int) -> Dict[str, torch.Tensor]:
        """The ensemble mean, scattered from class order back to shard order."""
        acc = torch.empty_like(self.accum).index_copy_(0, self.q_order, self.accum)
        return {"nn": ensemble_mean(acc, K)}


class KNNScore:
    """The per-call state of the knn scores (`methods`: those requested among KNN_METHODS) for the
    shard's `labels` [n] and k neighbours, built once and reused by every checkpoint.  The
    queries are the shard's rows in shard order with ids arange(n) + the shard's offset, the
    candidates every rank's rows in dataset order with ids arange(N) and every rank's labels
    (`rows`); `bad` is this shard's count of labels outside [0, C).  Holds the accumulators and
    the kernel's workspace (4 (n + N) pad16(D) + 4 N + 8 n splits k bytes).  A dataset of
    N <= k rows is rejected by name."""

    def __init__(self, methods, labels: torch.Tensor, linear, rows: GatheredRows, operands: str,
                 k: int):
        n, dev = labels.numel(), labels.device
        C, D = linear.out_features, linear.in_features
        _check_width("knn", D)
        N = sum(rows.lengths)
        check_knn_size(N, k)
        self.operands, self.k = operands, int(k)
        _, self.bad = _capi.class_counts(labels, C, check=False)
        self.q_id = torch.arange(n, dtype=torch.int64, device=dev) + rows.offset
        self.c_id = self.q_id if rows.local else torch.arange(N, dtype=torch.int64, device=dev)
        self.q_label, self.c_label = labels, rows.labels.contiguous()
        self.acc = {m: torch.zeros(n, dtype=torch.float32, device=dev) for m in methods}
        need = _capi.knn_workspace_bytes(n, N, D, self.k, 0, operands)
        self.workspace = torch.empty(max(need, 1), dtype=torch.uint8, device=dev)

    def end_checkpoint(self, features: torch.Tensor, allf: torch.Tensor):
        """At the same point of a checkpoint as NNScore's, on the same gathered rows `allf`: one
        dd_knn launch that accumulates the requested scores."""
        self.workspace = _capi.knn(
            features, self.q_id, allf, self.c_id, self.k, q_label=self.q_label,
            c_label=self.c_label, operands=self.operands, accum_dist=self.acc.get("knn"),
            accum_disagree=self.acc.get("knn_disagree"), workspace=self.workspace)

    def finalize(self, K: int) -> Dict[str, torch.Tensor]:
        return {m: ensemble_mean(a, K) for m, a in self.acc.items()}


class KDEScore:
    """The per-call state of the density scores (`methods`: those requested among DENSITY_METHODS)
    for the shard's `labels` [n], built once and reused by every checkpoint.  Queries, candidates,
    ids and labels as KNNScore's; `bad` is this shard's count of labels outside [0, C).  With
    kde_post the whole dataset's class counts are read to the host once: a class of exactly one
    member is rejected by name.  Holds the accumulators (of -ln sum w and of kde_post) and the
    kernel's workspace (4 (n + N) pad16(D) + 4 (n + N) + 16 n segments bytes).  Every rank
    computes the scale s from ALL the gathered rows in dataset order (kde_scale: one read back
    per checkpoint), so the scores do not depend on the chunk size, the lanes or the world
    size."""

    def __init__(self, methods, labels: torch.Tensor, linear, rows: GatheredRows, operands: str,
                 bandwidth: float):
        n, dev = labels.numel(), labels.device
        C, D = linear.out_features, linear.in_features
        _check_width("kde", D)
        self.N = sum(rows.lengths)
        self.operands, self.bandwidth = operands, float(bandwidth)
        _, self.bad = _capi.class_counts(labels, C, check=False)
        self.q_id = torch.arange(n, dtype=torch.int64, device=dev) + rows.offset
        self.c_id = (self.q_id if rows.local
                     else torch.arange(self.N, dtype=torch.int64, device=dev))
        self.q_label, self.c_label = labels, rows.labels.contiguous()
        if "kde_post" in methods:
            counts, _ = _capi.class_counts(self.c_label, C, check=False)
            check_no_singleton_class(counts.tolist(), "kde_post")  # the one read of the counts
        self.acc = {m: torch.zeros(n, dtype=torch.float32, device=dev) for m in methods}
        need = _capi.kde_workspace_bytes(n, self.N, D, 0, operands)
        self.workspace = torch.empty(max(need, 1), dtype=torch.uint8, device=dev)

    def end_checkpoint(self, features: torch.Tensor, allf: torch.Tensor):
        """At the same point of a checkpoint as NNScore's, on the same gathered rows `allf`: the
        scale, then one dd_kde launch that accumulates the requested scores."""
        inv = 1.0 / (self.bandwidth * kde_scale(allf))
        self.workspace = _capi.kde(
            features, self.q_id, allf, self.c_id, inv, q_label=self.q_label,
            c_label=self.c_label, operands=self.operands, accum_nll=self.acc.get("kde"),
            accum_post=self.acc.get("kde_post"), workspace=self.workspace)

    def finalize(self, K: int) -> Dict[str, torch.Tensor]:
        """The ensemble means; kde = ln(N - 1) - ln sum w: the constant is added once."""
        out = {m: ensemble_mean(a, K) for m, a in self.acc.items()}
        if "kde" in out:
            out["kde"] = out["kde"] + math.log(max(self.N - 1, 1))
        return out


class MahaScore:
    """The per-call state of the maha score for the shard's `labels` [n], built once and reused by
    every checkpoint: every rank's labels (`rows`), their class counts (`bad` is this shard's
    count of labels outside [0, C)) and label-sorted order, the accumulator and the kernels'
    workspace.  Every rank forms the class means and the scatter from ALL the gathered rows in
    dataset order and factors the same matrix, so nothing floating-point is reduced across ranks
    and the scores do not depend on the chunk size, the lanes or the world size.  With `proto`
    (the call's ProtoScore, when that score is requested too) the class means are not formed a
    second time: its `centroids` and `bad_feat` of the checkpoint are read (the same kernels on
    the same exact sums: the same bits)."""

    def __init__(self, labels: torch.Tensor, linear, rows: GatheredRows, operands: str,
                 shrink: float, proto: Optional["ProtoScore"] = None):
        n, dev = labels.numel(), labels.device
        C, D = linear.out_features, linear.in_features
        _check_width("maha", D)
        self.operands, self.shrink, self.proto = operands, float(shrink), proto
        self.labels, self.all_labels = labels, rows.labels.contiguous()
        self.N = self.all_labels.numel()
        _, self.bad = _capi.class_counts(labels, C, check=False)
        self.counts, _ = _capi.class_counts(self.all_labels, C, check=False)
        if self.N >= _capi.PROTO_MAX_CLASS:  # (the class means' fixed-point sums: proto's limit)
            check_class_sizes(int(self.counts.max().item()))
        self.order = torch.argsort(self.all_labels, stable=True)
        self.accum = torch.zeros(n, dtype=torch.float32, device=dev)
        need = _capi.maha_workspace_bytes(self.N, D, operands)
        self.workspace = torch.empty(max(need, 1), dtype=torch.uint8, device=dev)

    def end_checkpoint(self, features: torch.Tensor, allf: torch.Tensor):
        """At the same point of a checkpoint as NNScore's (after ProtoScore's), on the same
        gathered rows `allf`: the class means (ProtoScore's where it ran) and the scatter over all
        of them, the host's D x D algebra (which reads S
        and the two counters back: one synchronisation per checkpoint), and the distance launch
        over this shard's rows."""
        if self.proto is not None:
            mean, bad_feat = self.proto.centroids, self.proto.bad_feat
        else:
            mean, bad_feat = class_means(allf, self.all_labels, self.counts, self.order)
        S, nonfinite, self.workspace = _capi.maha_scatter(
            allf, self.all_labels, self.counts, mean, operands=self.operands,
            workspace=self.workspace)
        check_maha_rows(bad_feat, nonfinite)
        W = maha_whitener(S, self.N, self.shrink)
        _capi.maha_dist(features, self.labels, self.counts, mean, W, operands=self.operands,
                        accum=self.accum, workspace=self.workspace)

    def finalize(self, K: int) -> Dict[str, torch.Tensor]:
        return {"maha": ensemble_mean(self.accum, K)}


class ForwardScores:
    """Everything one score_shard call takes from the EL2N pass: the requested forward scores
    among cfg.methods (a ScoreConfig) for the shard's `labels` [n] and classifier `linear`.

    `counter` is the call's counter of labels outside [0, C) if the EL2N pass is the first over
    the shard, else None (the GraNd pass counts).  Each row is counted once: by a logit kernel
    on the first checkpoint if a logit member is requested, otherwise by adding dd_class_counts'
    `bad` of the shard's labels here."""

    def __init__(self, cfg, labels: torch.Tensor, linear, group=None,
                 counter: Optional[torch.Tensor] = None, kcenter_ckpt: Optional[int] = None):
        n, methods = labels.numel(), cfg.methods
        # the row-based selections (ScoreConfig.select_fill "kcenter", select_diversity "d2"):
        # every rank's feature rows of checkpoint `kcenter_ckpt` (0-based) are kept for run()'s
        # selection
        self.kcenter_ckpt, self.kcenter_rows, self._ckpts_done = kcenter_ckpt, None, 0
        logit = [m for m in methods if m in LOGIT_FAMILY]
        self.logit = LogitScores(logit, n, labels.device) if logit else None
        self.proto = self.kmeans = self.nn = self.knn = self.maha = self.kde = self.rows = None
        if "proto" in methods:
            self.proto = ProtoScore(labels, linear, group, cfg.batch_size)
        knn = [m for m in methods if m in KNN_METHODS]
        kde = [m for m in methods if m in DENSITY_METHODS]
        if "nn" in methods or knn or kde or "maha" in methods or kcenter_ckpt is not None:
            labels = labels.contiguous()
            self.rows = GatheredRows(labels, group)
        if "nn" in methods:
            self.nn = NNScore(labels, linear, self.rows, cfg.el2n_operands)
        if knn:
            self.knn = KNNScore(knn, labels, linear, self.rows, cfg.el2n_operands, cfg.knn_k)
        if kde:
            self.kde = KDEScore(kde, labels, linear, self.rows, cfg.el2n_operands,
                                cfg.kde_bandwidth)
        if "maha" in methods:
            self.maha = MahaScore(labels, linear, self.rows, cfg.el2n_operands, cfg.maha_shrink,
                                  self.proto)
        if "kmeans" in methods:
            lengths, rank = ((self.rows.lengths, self.rows.rank) if self.rows is not None
                             else shard_lengths(n, group))
            self.kmeans = KMeansScore(labels, linear, group, lengths, rank, cfg.el2n_operands,
                                      cfg.kmeans_k, cfg.kmeans_iters)
        # the one [n, D] fp32 buffer of the checkpoint's feature rows (n D 4 bytes: 102 MB at
        # 50 000 x 512, 10.5 GB for 1.28 M x 2048 rows on one rank), or None: logits only
        self.features = None
        by_features = (self.proto or self.nn or self.knn or self.kde or self.kmeans
                       or self.maha)
        if kcenter_ckpt is not None:
            _check_width("d2" if cfg.select_diversity == "d2" else "kcenter", linear.in_features)
        if by_features or kcenter_ckpt is not None:
            self.features = torch.empty((n, linear.in_features), dtype=torch.float32,
                                        device=labels.device)
        self._counter = counter if self.logit is not None else None
        if counter is not None and self.logit is None and by_features:
            counter.add_(by_features.bad)  # no logit kernel runs to count them

    def consume(self, ckpt_index: int, logits, labels, r0: int, r1: int):
        """One launch's logits (and labels) of rows [r0, r1) of the shard."""
        if self.logit is not None:
            self.logit.consume(ckpt_index, logits, labels, r0, r1,
                               self._counter if ckpt_index == 0 else None)

    def end_checkpoint(self):
        """The second phase of a checkpoint, on the current stream, once `features` holds every
        row of the shard; the next checkpoint's chunks, which overwrite `features`, must be
        ordered after it."""
        if self.proto is not None:
            self.proto.end_checkpoint(self.features)
        if self.kmeans is not None:
            self.kmeans.end_checkpoint(self.features)
        keep = self._ckpts_done == self.kcenter_ckpt
        # one all-gather of the rows serves nn, the knn scores, maha and the kcenter fill (which
        # alone needs it at its one checkpoint only)
        if self.rows is not None and (keep or self.nn is not None or self.knn is not None
                                      or self.kde is not None or self.maha is not None):
            allf = self.rows.gather(self.features)
            if keep:
                # (one rank: `allf` is the feature buffer itself, which the next checkpoint
                # overwrites)
                self.kcenter_rows = allf.clone() if allf is self.features else allf
            if self.nn is not None:
                self.nn.end_checkpoint(self.features, allf)
            if self.knn is not None:
                self.knn.end_checkpoint(self.features, allf)
            if self.kde is not None:
                self.kde.end_checkpoint(self.features, allf)
            if self.maha is not None:
                self.maha.end_checkpoint(self.features, allf)
        self._ckpts_done += 1

    def _parts(self):
        return [p for p in (self.logit, self.proto, self.nn, self.knn, self.kde, self.kmeans,
                            self.maha) if p is not None]

    def tensors(self) -> List[torch.Tensor]:
        """Every device buffer the pass and the second phase touch (for the streams'
        record_stream bookkeeping)."""
        return _tensors(self) + [t for p in self._parts() for t in _tensors(p)]

    def finalize(self, K: int) -> Dict[str, torch.Tensor]:
        """{method: fp32 [n]}, the ensemble scores over the K checkpoints consumed."""
        out = {}
        for p in self._parts():
            out.update(p.finalize(K))
        return out
