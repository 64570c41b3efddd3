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


def known(method: str) -> bool:
    return method == "grand" or method in FORWARD_SCORES or method in KNN_METHODS


def pass_of(method: str) -> str:
    """The pass that computes `method`: "el2n" (the shared forward of the logit family, the
    feature scores and the neighbour scores) or "grand"."""
    return "el2n" if method in FORWARD_SCORES or method in KNN_METHODS else "grand"


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


def seed_counts(quotas, seed_frac: float):
    """Seeds per group of the kcenter fill: max(1, floor(seed_frac * q)) for a quota q > 0, none
    for q = 0 (never more than q: seed_frac <= 1)."""
    return [max(1, int(np.floor(float(seed_frac) * int(q)))) if int(q) > 0 else 0 for q in quotas]
