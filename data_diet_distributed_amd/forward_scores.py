"""The consumers of the EL2N pass's train-BN forward: LogitScores (el2n + LOGIT_METHODS, from
each launch's logits), ProtoScore, NNScore and KNNScore (from the checkpoint's pooled feature
rows, over every rank), and ForwardScores, which holds the requested ones for one score_shard
call.

The pass hands every launch's logits to `consume` and, when `features` is not None, writes the
launch's feature rows there; after a checkpoint's last chunk it calls `end_checkpoint`.  Every
rank issues its collectives in the same order: the counts all-reduce (proto) and the lengths and
labels all-gathers (nn and the knn scores: one of each, shared, GatheredRows) at construction,
then per checkpoint the proto all-reduce followed by the one all-gather of the feature rows that
nn and the knn scores share.
"""
from __future__ import annotations

from typing import Dict, List, Optional

import torch

from . import _capi
from .collectives import _all_reduce_sum, gather_rows, shard_lengths, world_of
from .methods import KNN_METHODS, LOGIT_FAMILY


def check_class_sizes(largest: int):
    """The proto score's fixed-point class sums (|q| < 2^39 per element, int64) hold fewer than
    2^24 members per class: reject a larger class."""
    if largest >= _capi.PROTO_MAX_CLASS:
        raise ValueError(f"proto: a class of {largest} members; the exact int64 feature sums "
                         f"hold fewer than {_capi.PROTO_MAX_CLASS} (2^24) per class")


def check_no_singleton_class(counts):
    """The nn score of a class's only member would be infinite (no other row of its class):
    reject a dataset with such a class, naming it.  counts: members per class over the whole
    dataset (an empty class is fine)."""
    for c, m in enumerate(counts):
        if int(m) == 1:
            raise ValueError(f"nn: class {c} has exactly one member in the whole dataset; its "
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
        # the kcenter fill (ScoreConfig.select_fill): every rank's feature rows of checkpoint
        # `kcenter_ckpt` (0-based) are kept for run()'s selection
        self.kcenter_ckpt, self.kcenter_rows, self._ckpts_done = kcenter_ckpt, None, 0
        logit = [m for m in methods if m in LOGIT_FAMILY]
        self.logit = LogitScores(logit, n, labels.device) if logit else None
        self.proto = self.nn = self.knn = self.rows = None
        if "proto" in methods:
            self.proto = ProtoScore(labels, linear, group, cfg.batch_size)
        knn = [m for m in methods if m in KNN_METHODS]
        if "nn" in methods or knn or kcenter_ckpt is not None:
            labels = labels.contiguous()
            self.rows = GatheredRows(labels, group)
        if "nn" in methods:
            self.nn = NNScore(labels, linear, self.rows, cfg.el2n_operands)
        if knn:
            self.knn = KNNScore(knn, labels, linear, self.rows, cfg.el2n_operands, cfg.knn_k)
        # the one [n, D] fp32 buffer of the checkpoint's feature rows (n D 4 bytes: 102 MB at
        # 50 000 x 512, 10.5 GB for 1.28 M x 2048 rows on one rank), or None: logits only
        self.features = None
        by_features = self.proto or self.nn or self.knn
        if kcenter_ckpt is not None:
            _check_width("kcenter", linear.in_features)
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
        keep = self._ckpts_done == self.kcenter_ckpt
        # one all-gather of the rows serves nn, the knn scores and the kcenter fill (which alone
        # needs it at its one checkpoint only)
        if self.rows is not None and (keep or self.nn is not None or self.knn is not None):
            allf = self.rows.gather(self.features)
            if keep:
                # (one rank: `allf` is the feature buffer itself, which the next checkpoint
                # overwrites)
                self.kcenter_rows = allf.clone() if allf is self.features else allf
            if self.nn is not None:
                self.nn.end_checkpoint(self.features, allf)
            if self.knn is not None:
                self.knn.end_checkpoint(self.features, allf)
        self._ckpts_done += 1

    def _parts(self):
        return [p for p in (self.logit, self.proto, self.nn, self.knn) if p is not None]

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
