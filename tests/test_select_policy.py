"""Keep-set selection policies on the host: `apportion`, the config plumbing, and the NumPy
restatement of the selection contract that the GPU tests compare the kernels against.

Contract: class c has n_c members ranked by score descending, ties by ascending index (NaN
below every number, +0.0 == -0.0); with integer per-class skips s_c and quotas q_c the kept
examples of class c are its in-class ranks [s_c, s_c + q_c), and the output lists every kept
index ordered by score descending, ties by ascending index, over the whole set.
s = apportion(skip, n, rule), q = apportion(k, n - s, rule).
"""
import os
import random

import numpy as np
import pytest

from data_diet_distributed_amd import _capi, config as config_mod, score as score_mod
from data_diet_distributed_amd.scoring import ScoreConfig, apportion
from oracle import el2n as o_el2n

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- the NumPy restatement (imported by the GPU test modules) ---------------------------------
def ref_order(keys) -> np.ndarray:
    """Every index, by key descending, ties by ascending index; NaN after every number."""
    s = np.asarray(keys, dtype=np.float64)
    nan = np.isnan(s)
    neg = np.where(nan, 0.0, -s)
    return np.lexsort((np.arange(len(s)), neg, nan)).astype(np.int64)  # last key is primary


def ref_select_by_class(keys, labels, num_classes, class_skip, class_quota) -> np.ndarray:
    """Class c keeps its in-class ranks [class_skip[c], class_skip[c] + class_quota[c]); the
    kept indices in the global order."""
    order = ref_order(keys)
    cls = np.asarray(labels, dtype=np.int64)[order]
    counts = np.bincount(cls, minlength=num_classes)
    starts = np.cumsum(counts) - counts
    by_class = np.argsort(cls, kind="stable")
    rank = np.empty(len(order), dtype=np.int64)
    rank[by_class] = np.arange(len(order)) - starts[cls[by_class]]
    s = np.asarray(class_skip, dtype=np.int64)[cls]
    q = np.asarray(class_quota, dtype=np.int64)[cls]
    return order[(rank >= s) & (rank < s + q)]


def ref_quotas(labels, num_classes, k, policy, skip=0):
    """(per-class skips, per-class quotas) of a class policy."""
    n_c = np.bincount(np.asarray(labels, dtype=np.int64), minlength=num_classes).tolist()
    s = apportion(skip, n_c, policy)
    q = apportion(k, [a - b for a, b in zip(n_c, s)], policy)
    return s, q


def ref_select(keys, labels, num_classes, k, policy="global", skip=0) -> np.ndarray:
    """The keep-set of a policy."""
    if policy == "global":
        return ref_order(keys)[skip:skip + k]
    s, q = ref_quotas(labels, num_classes, k, policy, skip)
    return ref_select_by_class(keys, labels, num_classes, s, q)


# ---- apportion ---------------------------------------------------------------------------------
def test_apportion_worked_examples():
    assert apportion(7, [3, 3, 3], "stratified") == [3, 2, 2]
    assert apportion(5, [1, 2, 4], "stratified") == [1, 1, 3]
    assert apportion(7, [1, 10, 10], "balanced") == [1, 3, 3]
    assert apportion(5, [0, 4, 4, 4], "balanced") == [0, 2, 2, 1]


@pytest.mark.parametrize("rule", ["stratified", "balanced"])
def test_apportion_properties(rule):
    rng = random.Random(1234)
    for case in range(20000):
        C = rng.randint(1, 12)
        big = rng.random() < 0.1
        caps = [rng.randint(0, 10 ** 12 if big else 20) for _ in range(C)]
        M = sum(caps)
        total = rng.choice([0, M, rng.randint(0, M)])
        a = apportion(total, caps, rule)
        assert all(isinstance(v, int) for v in a)
        assert sum(a) == total, (total, caps)
        assert all(0 <= v <= c for v, c in zip(a, caps)), (total, caps, a)
        if total == M:
            assert a == caps
        if total == 0:
            assert a == [0] * C
        if rule == "balanced" and total < M:
            # water-filling: a class below the level is full; the others differ by at most one
            top = max(a)
            assert all(v == c or v >= top - 1 for v, c in zip(a, caps)), (total, caps, a)
    for C in (1, 2, 5, 10):
        for cap in (1, 7, 100):
            for total in range(0, C * cap + 1, max(1, C * cap // 7)):
                a = apportion(total, [cap] * C, rule)
                assert sum(a) == total and max(a) - min(a) <= 1
                if total % C == 0:
                    assert a == [total // C] * C
                assert a == sorted(a, reverse=True)  # the left-over units go to the lower ids


@pytest.mark.parametrize("rule", ["stratified", "balanced"])
def test_apportion_rejects_more_than_the_capacity(rule):
    with pytest.raises(ValueError):
        apportion(10, [3, 3, 3], rule)
    with pytest.raises(ValueError):
        apportion(1, [], rule)
    with pytest.raises(ValueError):
        apportion(-1, [3], rule)
    assert apportion(0, [], rule) == []


def test_apportion_rejects_unknown_rule():
    with pytest.raises(ValueError):
        apportion(1, [3], "global")


# ---- configuration -----------------------------------------------------------------------------
def test_score_config_validates_the_selection_fields():
    c = ScoreConfig()
    assert c.select_policy == "global" and c.select_skip == 0 and c.default_selection()
    assert ScoreConfig(select_policy="balanced", select_skip=3).select_skip == 3
    with pytest.raises(ValueError):
        ScoreConfig(select_policy="per_class")
    with pytest.raises(ValueError):
        ScoreConfig(select_skip=-1)
    with pytest.raises(ValueError):
        ScoreConfig(select_skip=1.5)
    for kw in ({"select_policy": "stratified"}, {"select_policy": "balanced"},
               {"select_skip": 5}):
        with pytest.raises(ValueError, match="refine"):
            ScoreConfig(refine=True, **kw)
        assert not ScoreConfig(refine="auto", **kw).default_selection()
        ScoreConfig(refine=False, **kw)
    ScoreConfig(refine=True)  # the default selection still takes it


def test_engine_config_maps_the_selection_keys():
    base = {"batch_size": 128}
    e = score_mod.engine_config(base)
    assert e.select_policy == "global" and e.select_skip == 0
    e = score_mod.engine_config(dict(base, select_policy="balanced", select_skip=7))
    assert e.select_policy == "balanced" and e.select_skip == 7
    with pytest.raises(ValueError):
        score_mod.engine_config(dict(base, select_policy="nope"))


def test_shipped_config_keeps_the_default_selection():
    cfg = config_mod.load_config(os.path.join(ROOT, "config.yaml"))
    assert cfg["select_policy"] == "global" and cfg["select_skip"] == 0
    assert config_mod.DEFAULTS["select_policy"] == "global"
    assert config_mod.DEFAULTS["select_skip"] == 0


def test_cli_overrides_parse():
    a = score_mod.parse(["--policy", "stratified", "--skip", "12"])
    assert a.policy == "stratified" and a.skip == 12
    a = score_mod.parse([])
    assert a.policy is None and a.skip is None


# ---- the restatement against the oracle's global rule -------------------------------------------
def test_restatement_with_one_class_is_the_global_rule():
    rng = np.random.default_rng(0)
    vals = np.array([0.5, 0.25, 0.0, -0.0, 1.0, 3.0, -2.0], dtype=np.float32)
    for keys in (rng.random(1000, dtype=np.float32), vals[rng.integers(0, len(vals), 1000)]):
        n = len(keys)
        labels = np.zeros(n, dtype=np.int64)
        for skip, k in ((0, 0), (0, 1), (0, n), (5, 100), (100, n - 100), (n, 0)):
            want = o_el2n.stable_topk(keys, skip + k)[skip:]
            for policy in ("global", "stratified", "balanced"):
                assert np.array_equal(ref_select(keys, labels, 1, k, policy, skip), want)
            assert np.array_equal(ref_select_by_class(keys, labels, 1, [skip], [k]), want)


def test_restatement_ranks_within_classes():
    keys = np.array([5, 1, 5, 3, np.nan, 2, 3, -np.inf], dtype=np.float32)
    labels = np.array([0, 0, 1, 1, 1, 0, 1, 1])
    assert ref_order(keys).tolist() == [0, 2, 3, 6, 5, 1, 7, 4]
    # class 0 ranks: 0, 5, 1; class 1 ranks: 2, 3, 6, 7, 4 (NaN last)
    assert ref_select_by_class(keys, labels, 2, [1, 0], [2, 2]).tolist() == [2, 3, 5, 1]
    assert ref_select_by_class(keys, labels, 2, [0, 3], [0, 2]).tolist() == [7, 4]
    assert ref_select(keys, labels, 2, 4, "balanced").tolist() == [0, 2, 3, 5]
    assert ref_quotas(labels, 2, 4, "stratified", skip=2) == ([1, 1], [1, 3])


# ---- the binding surface (loads on a CPU-only host) ---------------------------------------------
NEW_SYMBOLS = ("dd_class_counts", "dd_select_by_class_workspace_bytes",
               "dd_select_topk_by_class")


def test_new_entry_points_are_bound_and_exported():
    L = _capi.lib()
    for name in NEW_SYMBOLS:
        assert name in _capi.EXPORTS
        assert hasattr(L, name), name
    assert L.dd_abi_version() == 10  # additive: the version does not move
    for fn in ("class_counts", "select_topk_by_class", "select_by_class_workspace_bytes"):
        assert callable(getattr(_capi, fn))


def test_new_entry_points_validate_before_launching():
    import ctypes
    L = _capi.lib()
    P16 = ctypes.c_void_p(16)
    # the order (n int64), the flags and dd_select_topk's own workspace are all inside
    n, C = 50000, 10
    need = _capi.select_by_class_workspace_bytes(n, C)
    assert need > _capi.select_workspace_bytes(n) + 9 * n
    assert _capi.select_by_class_workspace_bytes(n, 70000) > need
    assert _capi.select_by_class_workspace_bytes(0, 1) > 0
    assert _capi.select_by_class_workspace_bytes(-1, 10) == 0
    assert _capi.select_by_class_workspace_bytes(n, 0) == 0
    assert _capi.select_by_class_workspace_bytes(1 << 31, 10) == 0
    assert L.dd_select_topk_by_class(P16, P16, 10, 3, P16, P16, 11, P16, None, P16, P16, 1 << 30,
                                     None) == -1
    assert b"k_total" in L.dd_last_error()
    assert L.dd_select_topk_by_class(P16, P16, 10, 0, P16, P16, 5, P16, None, P16, P16, 1 << 30,
                                     None) == -1
    assert b"num_classes" in L.dd_last_error()
    assert L.dd_select_topk_by_class(P16, P16, 10, 3, P16, P16, 5, P16, None, None, P16, 1 << 30,
                                     None) == -1
    assert L.dd_select_topk_by_class(P16, P16, 10, 3, P16, P16, 5, P16, None, P16, P16, 64,
                                     None) == -3  # workspace too small, before any launch
    assert L.dd_class_counts(P16, -1, 3, P16, P16, None) == -1
    assert L.dd_class_counts(P16, 10, 0, P16, P16, None) == -1
    assert L.dd_class_counts(P16, 10, 3, None, P16, None) == -1
