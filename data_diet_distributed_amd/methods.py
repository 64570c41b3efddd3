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


def check_selection(policy, skip, policy_name="select_policy", skip_name="select_skip") -> int:
    """The selection fields of ScoreConfig, and sparse_loader's `policy` / `skip` under their
    own names: a known policy and an integer skip >= 0 (returned as an int)."""
    if policy not in SELECT_POLICIES:
        raise ValueError(f"{policy_name} must be one of {SELECT_POLICIES} (got {policy!r})")
    if isinstance(skip, bool) or not isinstance(skip, (int, np.integer)) or skip < 0:
        raise ValueError(f"{skip_name} must be an integer >= 0 (got {skip!r})")
    return int(skip)
