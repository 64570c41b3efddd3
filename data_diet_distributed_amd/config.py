"""config.yaml handling: the reference's 14 keys stay accepted, new keys get defaults.

Reference keys (config.yaml:1-14), read by train.py:36-49 / ddp.py:54-62.  `sparsity` (:3)
and `batch_size_scores` (:4) are never read by the reference (the CLI `--sparsity` wins and
scoring uses `batch_size`); they are kept and ignored the same way.
"""
from __future__ import annotations

import yaml

REFERENCE_KEYS = ("device", "sparse", "sparsity", "batch_size_scores", "num_workers", "dataset",
                  "batch_size", "start_epoch", "num_epochs", "lr", "momentum", "weight_decay",
                  "checkpoint_path", "sparse_checkpoint_path")

# build extensions (defaults reproduce the reference: EL2N, one checkpoint ckpt_19, train BN)
DEFAULTS = {
    # el2n and/or grand and/or the other logit scores of the EL2N forward: loss | margin |
    # entropy | error | wrong_mass | variability (scoring.LOGIT_METHODS) | proto (the distance
    # to the class prototype in feature space, scoring.FEATURE_METHODS) | nn (the distance to
    # the nearest other example of the same class, scoring.NEIGHBOR_METHODS) | knn, knn_disagree
    # (the mean distance to the knn_k nearest other examples of any class and the share of them
    # with another label, scoring.KNN_METHODS) | kmeans (the distance to the nearest centroid of
    # a k-means clustering of the feature rows: the prototype distance without labels,
    # scoring.CLUSTER_METHODS) | maha (the Mahalanobis distance to the class mean under the tied
    # within-class covariance of the feature rows, scoring.COVARIANCE_METHODS) | kde, kde_post (the
    # negative log kernel density among all feature rows and the negative log Parzen posterior of
    # the own label, scoring.DENSITY_METHODS); select_by takes any
    "score_methods": ["el2n"],
    "select_by": "el2n",
    "knn_k": 5,                       # neighbours of knn / knn_disagree (1..16)
    "kmeans_k": 0,                    # clusters of kmeans (0: num_classes; at most 4096)
    "kmeans_iters": 20,               # Lloyd updates of kmeans per checkpoint (1..1000)
    "maha_shrink": 0.01,              # shrinkage of maha's covariance to its mean eigenvalue [0, 1]
    "kde_bandwidth": 0.25,            # kde / kde_post: bandwidth^2 over the mean squared distance (> 0)
    "select_policy": "global",        # global (reference) | stratified | balanced class quotas
    "select_skip": 0,                 # ranks skipped from the top before the k kept ones
    "select_fill": "score",           # score (the rank cut) | kcenter (coverage: greedy k-center)
    "kcenter_seed_frac": 0.0,         # share of a quota seeded by the score (at least one seed)
    "kcenter_objective": "radius",    # radius (farthest-first) | inertia (greedy k-medoids)
    "kcenter_match": "none",          # none | mean (kernel herding: the kept mean tracks the group's)
    "kcenter_cover": "none",          # none | ball (greedy max coverage at a fixed radius)
    "cover_radius": 0.25,             # the ball's squared radius, a share of the group's mean
    #                                   squared pairwise distance (> 0; a convention, not tuned)
    "kcenter_ckpt": -1,              # the checkpoint whose feature rows the row-based
    #                                   selections read (the kcenter fill, the d2 diversity)
    "select_diversity": "none",       # none | d2 (D2 pruning: message passing on the kNN graph)
    "d2_k": 10,                       # neighbours per example of the d2 graph (1..16)
    "d2_gamma_f": 1.0,                # sharpness of the forward edge weights (>= 0)
    "d2_gamma_r": 1.0,                # sharpness of the reverse edge weights (>= 0)
    "score_checkpoints": 1,           # K (seed{k}/ckpt_{epoch}.pth when K > 1)
    "score_epoch": 19,
    "bn_mode": "batch",               # EL2N BN: batch (reference) | running (eval)
    "grand_batch": 1024,
    "pegrad_method": "auto",          # auto | direct | ghost
    "score_precision": "split",       # split (exact keep-set) | split_fast | bf16x3[_fast] | fp32
    "score_lanes": 3,                 # HIP streams the launch chunks are dealt to
    "refine_max_frac": 0.08,          # bf16x3: most of the set the fp32 re-scoring may take
    "score_gpus": 1,
    "subset_index_path": None,        # write the keep-set here when set
    "arch": "resnet18",
    "num_classes": 10,
}


def load_config(path: str) -> dict:
    with open(path) as f:
        cfg = yaml.safe_load(f) or {}
    out = dict(DEFAULTS)
    out.update(cfg)
    return out
