"""The score methods and the selection policies: what there is, and every fact about a method
that the engine, the config and the drop-in decide by (each decided here, once)."""
from __future__ import annotations

import numpy as np

from . import _capi

# The logit scores beside EL2N (include/dd_capi.h dd_logit_scores): the mean over the K
# checkpoints of the five single-forward statistics, and Dataset Cartography's variability, the
# standard deviation of wrong_mass over the checkpoints.  Larger means harder for every one.
LOGIT_METHODS = _capi.LOGIT_STATS + ("variability",)
LOGIT_FAMILY = ("el2n",) + LOGIT_METHODS  # the scores of one train-BN forward per checkpoint
# Scores of that forward's pooled feature rows f_i (the rows the classifier consumes):
#   proto_i = || f_i - mu_{y_i} ||_2,  mu_c = the mean of f_i over the WHOLE dataset's class c
# (Sorscher et al.'s prototypicality; larger = more atypical).  Not a function of one row: the
# class means are summed in exact fixed point over chunks, lanes and ranks (include/dd_capi.h
# dd_class_feature_sums), which keeps the scores bitwise independent of all three.
FEATURE_METHODS = ("proto",)
# everything the EL2N forward produces: one forward per checkpoint and chunk serves them all
FORWARD_FAMILY = LOGIT_FAMILY + FEATURE_METHODS
# Scores of a row against the other rows of its class, from the same feature rows:
#   nn_i = min over j != i with y_j == y_i, over the WHOLE dataset, of || f_i - f_j ||_2
# (the redundancy signal of SemDeDup and the density / coreset family: a near-duplicate scores
# close to 0, so the default policy, which keeps the largest scores, drops duplicates first).
NEIGHBOR_METHODS = ("nn",)
# every score that comes from the EL2N forward
FORWARD_SCORES = FORWARD_FAMILY + NEIGHBOR_METHODS
# Scores of a row against its k nearest other rows of ANY class (k = ScoreConfig.knn_k), from
# the same feature rows, the neighbourhood taken by (squared distance, example index):
#   knn_i          = the mean of || f_i - f_j ||_2 over the k neighbours j (the density / coverage
#                    measure of the coreset family; needs no labels)
#   knn_disagree_i = the share of the k neighbours with y_j != y_i (deep k-NN filtering: a
#                    mislabelled example sits among another class's rows)
# Larger = more isolated / more suspicious.  They come from the EL2N forward too; FORWARD_SCORES
# keeps its value and every decision goes through known() / pass_of().
KNN_METHODS = ("knn", "knn_disagree")
# The score of a row against the centroids of a k-means clustering of the WHOLE dataset's feature
# rows (ScoreConfig.kmeans_k clusters, kmeans_iters Lloyd updates from evenly spaced seed rows):
#   kmeans_i = || f_i - mu_{a(i)} ||_2, a(i) the nearest centroid
# (Sorscher et al.'s self-supervised prototype distance: proto without labels; larger = more
# atypical).  The cluster sums are exact fixed point like proto's, so the scores are bitwise
# independent of chunks, lanes and ranks (include/dd_capi.h dd_kmeans_assign).
CLUSTER_METHODS = ("kmeans",)
# proto's distance in the metric of the rows' own tied (within-class) covariance (Lee et al. 2018;
# shrinkage lambda = ScoreConfig.maha_shrink), from the same feature rows over the WHOLE dataset:
#   maha_i = || L^-1 (f_i - mu_{y_i}) ||_2,  L L^T = S / N + lambda (tr(S / N) / D) I,
#   S = sum_i (f_i - mu_{y_i}) (f_i - mu_{y_i})^T
# (larger = more atypical; no handful of high-variance channels carries the distance).  Every rank
# forms S from all the rows in dataset order, so the scores are bitwise independent of chunks,
# lanes and ranks (include/dd_capi.h dd_maha_scatter).
COVARIANCE_METHODS = ("maha",)
# The soft form of the KNN_METHODS, from the same feature rows over the WHOLE dataset: every other
# row votes with the weight w_ij = exp(-|| f_i - f_j ||^2 / (tau s)), tau = ScoreConfig.
# kde_bandwidth, s = the mean squared distance over all ordered pairs of distinct rows:
#   kde_i      = ln(N - 1) - ln sum_{j != i} w_ij (the negative log kernel density: coreset
#                density weighting; needs no labels)
#   kde_post_i = ln sum_{j != i} w_ij - ln sum_{j != i, y_j = y_i} w_ij (the negative log Parzen-
#                window posterior of the row's own label: knn_disagree with every row voting)
# Larger = more isolated / more suspicious.  No k and no hard cut (dd_kde: a streaming
# log-sum-exp over all N rows per row).
DENSITY_METHODS = ("kde", "kde_post")


def known(method: str) -> bool:
    return (method == "grand" or method in FORWARD_SCORES or method in KNN_METHODS
            or method in CLUSTER_METHODS or method in COVARIANCE_METHODS
            or method in DENSITY_METHODS)


def pass_of(method: str) -> str:
    """The pass that computes `method`: "el2n" (the shared forward of the logit family, the
    feature scores, the neighbour scores, the cluster score, the covariance score and the density
    scores) or "grand"."""
    return ("el2n" if method in FORWARD_SCORES or method in KNN_METHODS
            or method in CLUSTER_METHODS or method in COVARIANCE_METHODS
            or method in DENSITY_METHODS else "grand")


def check_shrink(shrink, name="maha_shrink") -> float:
    """ScoreConfig's maha_shrink, and sparse_loader's under its own name: a number in [0, 1]
    (returned as a float)."""
    if (isinstance(shrink, bool) or not isinstance(shrink, (int, float, np.integer, np.floating))
            or not 0.0 <= float(shrink) <= 1.0):
        raise ValueError(f"{name} must be a number in [0, 1] (got {shrink!r})")
    return float(shrink)


def check_bandwidth(bandwidth, name="kde_bandwidth") -> float:
    """ScoreConfig's kde_bandwidth, and sparse_loader's under its own name: a finite number > 0
    (returned as a float)."""
    if (isinstance(bandwidth, bool)
            or not isinstance(bandwidth, (int, float, np.integer, np.floating))
            or not 0.0 < float(bandwidth) < float("inf")):
        raise ValueError(f"{name} must be a finite number > 0 (got {bandwidth!r})")
    return float(bandwidth)


def refinable(method: str) -> bool:
    """Whether the fp32 refinement can re-score `method`: EL2N and GraNd only."""
    return method in ("el2n", "grand")


SELECT_POLICIES = ("global", "stratified", "balanced")


def check_selection(policy, skip, policy_name="select_policy", skip_name="select_skip",
                    fill="score", seed_frac=0.0, *, fill_name="select_fill",
                    frac_name="kcenter_seed_frac") -> int:
    """The selection fields of ScoreConfig, and sparse_loader's `policy` / `skip` / `fill` /
    `seed_frac` under their own names: a known policy, an integer skip >= 0 (returned as an int)
    and check_fill's conditions on the fill."""
    if policy not in SELECT_POLICIES:
        raise ValueError(f"{policy_name} must be one of {SELECT_POLICIES} (got {policy!r})")
    if isinstance(skip, bool) or not isinstance(skip, (int, np.integer)) or skip < 0:
        raise ValueError(f"{skip_name} must be an integer >= 0 (got {skip!r})")
    check_fill(fill, seed_frac, int(skip), fill_name=fill_name, frac_name=frac_name,
               skip_name=skip_name)
    return int(skip)


# How the keep-set is filled once the groups and quotas of the policy are fixed:
#   "score"    the rank cut on the select_by score (every policy above)
#   "kcenter"  coverage: each group's top max(1, floor(seed_frac * quota)) by the score seed a
#              farthest-first traversal of the group's feature rows (dd_kcenter_greedy), which
#              picks the rest: the k-center greedy of Sener & Savarese's core-set selection
SELECT_FILLS = ("score", "kcenter")


def check_fill(fill, seed_frac, skip=0, *, fill_name="select_fill",
               frac_name="kcenter_seed_frac", skip_name="select_skip") -> float:
    """ScoreConfig's select_fill / kcenter_seed_frac, and sparse_loader's `fill` / `seed_frac`
    under their own names: a known fill, a seed fraction in [0, 1] (returned as a float), and no
    skip with the kcenter fill."""
    if fill not in SELECT_FILLS:
        raise ValueError(f"{fill_name} must be one of {SELECT_FILLS} (got {fill!r})")
    if (isinstance(seed_frac, bool) or not isinstance(seed_frac, (int, float, np.integer,
                                                                  np.floating))
            or not 0.0 <= float(seed_frac) <= 1.0):
        raise ValueError(f"{frac_name} must be a number in [0, 1] (got {seed_frac!r})")
    if fill == "kcenter" and skip:
        raise ValueError(f"{fill_name}='kcenter' needs {skip_name}=0 (got {skip!r}): an offset "
                         f"window is a rank cut's notion")
    return float(seed_frac)


# What the centre-based fill ("kcenter") optimises once a group is seeded:
#   "radius"   the LARGEST distance from a dropped row to a kept one: farthest-first traversal
#              (dd_kcenter_greedy).  Its picks are each group's outliers.
#   "inertia"  the SUM of the squared distances of all rows to their nearest kept row: the greedy
#              k-medoids / facility-location rule (dd_kmedoids_greedy), each pick the row that
#              lowers the sum the most.  Its picks are representative rows of dense regions.
KCENTER_OBJECTIVES = ("radius", "inertia")


def check_objective(objective, name="kcenter_objective") -> str:
    """ScoreConfig's kcenter_objective, and select_with_policy's / sparse_loader's `objective`
    under their own name: one of KCENTER_OBJECTIVES, checked whatever the fill."""
    if objective not in KCENTER_OBJECTIVES:
        raise ValueError(f"{name} must be one of {KCENTER_OBJECTIVES} (got {objective!r})")
    return objective


# Whether the centre-based fill ("kcenter") matches a moment of its group instead of covering it:
#   "none"  the fill picks by kcenter_objective
#   "mean"  kernel herding (Welling; DeepCore's Herding, iCaRL's exemplar rule): every pick is the
#           row that brings the mean of the kept rows closest to the group's mean
#           (dd_herding_greedy).  The seeds, the groups and the quotas are the fill's.
KCENTER_MATCH = ("none", "mean")


def check_match(match, fill="kcenter", objective="radius", *, name="kcenter_match",
                fill_name="select_fill", objective_name="kcenter_objective") -> str:
    """ScoreConfig's kcenter_match, and select_with_policy's / sparse_loader's `match` under their
    own names: one of KCENTER_MATCH (checked whatever the fill); "mean" replaces the picks of the
    kcenter fill, so it needs that fill and the default objective."""
    if match not in KCENTER_MATCH:
        raise ValueError(f"{name} must be one of {KCENTER_MATCH} (got {match!r})")
    if match == "mean" and fill != "kcenter":
        raise ValueError(f"{name}='mean' needs {fill_name}='kcenter' (got {fill!r}): herding "
                         f"fills the quotas of the centre-based fill")
    if match == "mean" and objective != "radius":
        raise ValueError(f"{name}='mean' needs {objective_name}='radius', the default (got "
                         f"{objective!r}): the picks follow one rule")
    return match


# Whether the centre-based fill ("kcenter") covers at a FIXED radius instead of minimising one:
#   "none"  the fill picks by kcenter_objective / kcenter_match
#   "ball"  greedy maximum coverage (ProbCover, Yehuda et al.): with theta = cover_radius times
#           the group's mean squared pairwise distance, every pick is the row whose theta-ball
#           holds the most rows not yet within theta of a kept row, a tie to the better score
#           (dd_cover_greedy).  The seeds, the groups and the quotas are the fill's.
KCENTER_COVER = ("none", "ball")


def check_cover(cover, radius, fill="kcenter", objective="radius", match="none", *,
                name="kcenter_cover", radius_name="cover_radius", fill_name="select_fill",
                objective_name="kcenter_objective", match_name="kcenter_match"):
    """ScoreConfig's kcenter_cover and cover_radius, and select_with_policy's / sparse_loader's
    `cover` and `cover_radius` under their own names: one of KCENTER_COVER and a finite number
    > 0 (both checked whatever the fill); "ball" replaces the picks of the kcenter fill, so it
    needs that fill, the default objective and no match.  Returns (cover, radius as a float)."""
    if cover not in KCENTER_COVER:
        raise ValueError(f"{name} must be one of {KCENTER_COVER} (got {cover!r})")
    radius = check_bandwidth(radius, radius_name)
    if cover == "ball" and fill != "kcenter":
        raise ValueError(f"{name}='ball' needs {fill_name}='kcenter' (got {fill!r}): the cover "
                         f"fills the quotas of the centre-based fill")
    if cover == "ball" and objective != "radius":
        raise ValueError(f"{name}='ball' needs {objective_name}='radius', the default (got "
                         f"{objective!r}): the picks follow one rule")
    if cover == "ball" and match != "none":
        raise ValueError(f"{name}='ball' needs {match_name}='none', the default (got "
                         f"{match!r}): the picks follow one rule")
    return cover, radius


# Whether the rank cut (select_fill "score") also weighs coverage:
#   "none"  the rank cut as it is
#   "d2"    D2 pruning (Maharana, Yadav & Bansal): the examples sit on the d2_k-nearest-neighbour
#           graph of their feature rows (dd_knn, all classes), edge weights exp(-gamma d^2 / s)
#           with s the mean finite squared neighbour distance.  One round of forward message
#           passing lets a score absorb its neighbours' (weights by d2_gamma_f, dd_d2_propagate);
#           then the groups' quotas are filled greedily by the updated score, every pick lowering
#           its live neighbours' scores by weight x its own (weights by d2_gamma_r, dd_d2_select),
#           so the next pick moves elsewhere.  Both gammas large: every weight is 0 and the
#           keep-set is the rank cut's.
SELECT_DIVERSITY = ("none", "d2")


def check_diversity(diversity, k=10, gamma_f=1.0, gamma_r=1.0, fill="score", skip=0, *,
                    name="select_diversity", k_name="d2_k", gamma_f_name="d2_gamma_f",
                    gamma_r_name="d2_gamma_r", fill_name="select_fill",
                    skip_name="select_skip"):
    """ScoreConfig's select_diversity / d2_k / d2_gamma_f / d2_gamma_r, and select_with_policy's /
    sparse_loader's under their own names: a known diversity, 1 <= k <= _capi.KNN_MAX_K, finite
    gammas >= 0 (all checked whatever the diversity), and "d2" with the score fill and no skip.
    Returns (k, gamma_f, gamma_r) as an int and two floats."""
    if diversity not in SELECT_DIVERSITY:
        raise ValueError(f"{name} must be one of {SELECT_DIVERSITY} (got {diversity!r})")
    if (isinstance(k, bool) or not isinstance(k, (int, np.integer))
            or not 1 <= k <= _capi.KNN_MAX_K):
        raise ValueError(f"{k_name} must be an integer in 1..{_capi.KNN_MAX_K} (got {k!r})")
    for g_name, g in ((gamma_f_name, gamma_f), (gamma_r_name, gamma_r)):
        if (isinstance(g, bool) or not isinstance(g, (int, float, np.integer, np.floating))
                or not 0.0 <= float(g) < float("inf")):
            raise ValueError(f"{g_name} must be a finite number >= 0 (got {g!r})")
    if diversity == "d2" and fill != "score":
        raise ValueError(f"{name}='d2' needs {fill_name}='score' (got {fill!r}): the kcenter "
                         f"fill is a coverage rule of its own")
    if diversity == "d2" and skip:
        raise ValueError(f"{name}='d2' needs {skip_name}=0 (got {skip!r}): an offset window is "
                         f"a rank cut's notion")
    return int(k), float(gamma_f), float(gamma_r)


def seed_counts(quotas, seed_frac: float):
    """Seeds per group of the kcenter fill: max(1, floor(seed_frac * q)) for a quota q > 0, none
    for q = 0 (never more than q: seed_frac <= 1)."""
    return [max(1, int(np.floor(float(seed_frac) * int(q)))) if int(q) > 0 else 0 for q in quotas]
