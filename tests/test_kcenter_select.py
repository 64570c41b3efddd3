"""The coverage keep-set (ScoreConfig.select_fill = "kcenter") on the host: the float64
restatement of the greedy k-center fill that the device tests compare against, with checks of
its own, the config validation, the seed-count rule and the config / command-line plumbing.
"""
import ctypes
import itertools
import math

import numpy as np
import pytest

from data_diet_distributed_amd import _capi, config, methods, score
from data_diet_distributed_amd.scoring import ScoreConfig, ScoringEngine


def sq_dists64(f):
    """[n, n] float64 squared distances as sums of squared differences."""
    f = np.asarray(f, dtype=np.float64)
    return ((f[:, None, :] - f[None, :, :]) ** 2).sum(axis=2)


def ref_kcenter(f, ids, groups, seeds, quotas):
    """The kcenter fill in float64.  f [n, D]; ids [n] (distinct inside a group); groups [n]
    (a row outside [0, G) is in no group); seeds: indices of rows of f, the centres the groups
    start from; quotas [G]: the rows each group keeps in all, its seeds included.

    Group g takes quotas[g] - (its seeds) picks: each the not-yet-kept row of the group with
    the largest d2 = min over the group's kept rows of the squared distance, a tie to the
    smaller id.  Returns (picked int64 [steps, G], radius2 float64 [steps, G], mind2 float64
    [n]): picked[t, g] the id taken at step t and radius2[t, g] its d2 then (both -1 past the
    group's picks); mind2 the final d2 (-1: kept; +inf: nothing kept in the row's group)."""
    f = np.asarray(f, dtype=np.float64)
    ids, groups = np.asarray(ids, dtype=np.int64), np.asarray(groups, dtype=np.int64)
    seeds = np.asarray(seeds, dtype=np.int64)
    G, n = len(quotas), len(f)
    picks = [int(quotas[g]) - int((groups[seeds] == g).sum()) for g in range(G)]
    assert all(p >= 0 for p in picks)
    steps = max(picks) if picks else 0
    picked = np.full((steps, G), -1, dtype=np.int64)
    radius2 = np.full((steps, G), -1.0)
    mind2 = np.full(n, np.inf)
    for g in range(G):
        member = np.nonzero(groups == g)[0]
        kept = np.zeros(n, dtype=bool)
        for c in seeds[groups[seeds] == g]:
            mind2[member] = np.minimum(mind2[member], ((f[member] - f[c]) ** 2).sum(axis=1))
            kept[c] = True
        for t in range(picks[g]):
            open_ = member[~kept[member]]
            far = mind2[open_].max()
            tied = open_[mind2[open_] == far]
            c = tied[np.argmin(ids[tied])]
            picked[t, g], radius2[t, g] = ids[c], far
            kept[c] = True
            mind2[member] = np.minimum(mind2[member], ((f[member] - f[c]) ** 2).sum(axis=1))
        mind2[kept] = -1.0
    return picked, radius2, mind2


def check_greedy(f, ids, groups, seeds, picks, picked, slack=0.0):
    """The greedy property of `picked` [steps, G] in float64, group by group and step by step
    (none skipped): the row taken at step t has a min squared distance to the centres BEFORE
    it (the seeds and the earlier picks of ITS OWN run) of at least (1 - slack) times the
    largest over the group's unkept rows; it is a member, and not kept before.  Returns
    (the [steps, G] float64 min squared distances of the picks, -1 past a group's picks; the
    float64 [n] final min squared distances to that run's kept rows, -1 for a kept row, +inf
    for a row whose group keeps nothing)."""
    f = np.asarray(f, dtype=np.float64)
    ids, groups = np.asarray(ids), np.asarray(groups)
    seeds = np.asarray(seeds, dtype=np.int64)
    row_of = {(int(g), int(i)): r for r, (g, i) in enumerate(zip(groups, ids))}
    out = np.full(picked.shape, -1.0)
    final = np.full(len(f), np.inf)
    for g in range(picked.shape[1]):
        member = np.nonzero(groups == g)[0]
        local = {int(r): j for j, r in enumerate(member)}
        d2 = np.full(len(member), np.inf)
        kept = np.zeros(len(member), dtype=bool)

        def fold(r):
            np.minimum(d2, ((f[member] - f[r]) ** 2).sum(axis=1), out=d2)
            kept[local[r]] = True

        for c in seeds[groups[seeds] == g]:
            fold(int(c))
        assert np.all(picked[picks[g]:, g] == -1)
        for t in range(picks[g]):
            assert kept.any(), "a pick without a centre"
            r = row_of[(g, int(picked[t, g]))]  # a member of g (KeyError otherwise)
            assert not kept[local[r]], (g, t, "picked twice")
            mine, far = d2[local[r]], d2[~kept].max()
            assert mine >= (1.0 - slack) * far, (g, t, mine, far)
            out[t, g] = mine
            fold(r)
        d2[kept] = -1.0
        final[member] = d2
    return out, final


# ---- the restatement's own checks ----------------------------------------------------------
def test_ref_picks_are_greedy_and_never_repeat():
    rng = np.random.default_rng(3)
    n, D, G = 60, 7, 3
    f = rng.integers(-5, 6, size=(n, D)).astype(np.float32)
    f[17] = f[4]
    f[33] = f[4]  # duplicates: distance 0, never picked twice
    groups = rng.integers(0, G, size=n)
    ids = rng.permutation(n)
    sizes = [int((groups == g).sum()) for g in range(G)]
    seeds = np.array([np.nonzero(groups == g)[0][0] for g in range(G)])
    quotas = [sizes[0], 5, 1]  # a group kept whole, a partial one, seeds only
    picked, radius2, mind2 = ref_kcenter(f, ids, groups, seeds, quotas)
    picks = [q - 1 for q in quotas]
    got, final = check_greedy(f, ids, groups, seeds, picks, picked)
    assert np.array_equal(got, radius2) and np.array_equal(final, mind2)
    assert np.all(np.diff(radius2[:picks[0], 0]) <= 0)  # the radii never grow
    assert np.all(mind2[groups == 0] == -1)
    kept = np.concatenate([ids[seeds]] + [picked[:picks[g], g] for g in range(G)])
    assert len(kept) == sum(quotas)
    for g in range(G):
        mine = np.concatenate([ids[seeds[g:g + 1]], picked[:picks[g], g]])
        assert len(set(mine.tolist())) == quotas[g]
    # a tie goes to the smaller id: four corners of a square around a centre seed
    sq = np.array([[0, 0], [1, 1], [1, -1], [-1, 1], [-1, -1]], dtype=np.float32)
    p, r2, _ = ref_kcenter(sq, [9, 7, 3, 5, 4], [0] * 5, [0], [3])
    assert p[:, 0].tolist() == [3, 4] and r2[:, 0].tolist() == [2.0, 2.0]


def test_ref_radius_within_twice_the_optimum():
    """Gonzalez: farthest-first from ONE arbitrary centre covers within twice the optimal
    k-center radius (centres among the points).  Brute force over every k-subset at n <= 9."""
    rng = np.random.default_rng(11)
    for n, D, k in ((9, 2, 3), (8, 3, 4), (7, 1, 2), (9, 5, 5)):
        f = rng.normal(size=(n, D)).astype(np.float32)
        d = np.sqrt(sq_dists64(f))
        opt = min(d[:, list(S)].min(axis=1).max() for S in itertools.combinations(range(n), k))
        for seed in range(n):
            _, _, mind2 = ref_kcenter(f, np.arange(n), np.zeros(n, int), [seed], [k])
            radius = math.sqrt(mind2.max())
            assert (mind2 == -1).sum() == k
            assert radius <= 2 * opt * (1 + 1e-12), (n, k, seed, radius, opt)


# ---- configuration -------------------------------------------------------------------------
def test_score_config_validation():
    c = ScoreConfig()
    assert (c.select_fill, c.kcenter_seed_frac, c.kcenter_ckpt) == ("score", 0.0, -1)
    assert c.default_selection()
    assert methods.SELECT_FILLS == ("score", "kcenter")
    k = ScoreConfig(select_fill="kcenter", kcenter_seed_frac=0.25, select_policy="balanced")
    assert not k.default_selection() and k.refine == "auto"
    assert not ScoreConfig(select_fill="kcenter").default_selection()
    with pytest.raises(ValueError, match="select_fill"):
        ScoreConfig(select_fill="coverage")
    for bad in (-0.01, 1.5, float("nan"), "0.5", True):
        with pytest.raises(ValueError, match="kcenter_seed_frac"):
            ScoreConfig(select_fill="kcenter", kcenter_seed_frac=bad)
    with pytest.raises(ValueError, match="kcenter_seed_frac"):
        ScoreConfig(kcenter_seed_frac=2.0)  # checked whatever the fill
    with pytest.raises(ValueError, match="select_skip"):
        ScoreConfig(select_fill="kcenter", select_skip=3)
    with pytest.raises(ValueError, match="refine=True"):
        ScoreConfig(select_fill="kcenter", refine=True)
    with pytest.raises(ValueError, match="kcenter_ckpt"):
        ScoreConfig(select_fill="kcenter", kcenter_ckpt=0.5)
    assert ScoreConfig(select_fill="score", select_skip=3).select_skip == 3  # as before


def test_engine_range_checks_kcenter_ckpt():
    models = [object()] * 3  # rejected before anything looks at them
    for bad in (3, -4, 17):
        with pytest.raises(ValueError, match="kcenter_ckpt"):
            ScoringEngine(models, ScoreConfig(select_fill="kcenter", kcenter_ckpt=bad), "cuda:0")
    with pytest.raises(ValueError, match="EL2N forward"):
        ScoringEngine(models, ScoreConfig(methods=("grand",), select_by="grand",
                                          select_fill="kcenter"), "cuda:0")
    # in range: the next check is the device's (the engine has no CPU path)
    for ok in (-3, 0, 2):
        with pytest.raises(ValueError, match="GPU"):
            ScoringEngine(models, ScoreConfig(select_fill="kcenter", kcenter_ckpt=ok), "cpu")


def test_seed_count_rule():
    """m_g = max(1, floor(seed_frac * q_g)) for q_g > 0, and 0 for q_g = 0."""
    assert methods.seed_counts([0, 1, 2, 10, 25], 0.0) == [0, 1, 1, 1, 1]
    assert methods.seed_counts([0, 1, 2, 10, 25], 1.0) == [0, 1, 2, 10, 25]
    assert methods.seed_counts([0, 1, 9, 10, 25, 25000], 0.1) == [0, 1, 1, 1, 2, 2500]
    assert methods.seed_counts([3, 4, 5], 0.5) == [1, 2, 2]
    for frac in (0.0, 0.1, 0.33, 0.5, 0.999, 1.0):
        for q in range(0, 40):
            m = methods.seed_counts([q], frac)[0]
            assert m == (max(1, math.floor(frac * q)) if q else 0) and m <= q


def test_check_selection_learns_the_fill():
    assert methods.check_selection("global", 0, fill="kcenter", seed_frac=0.5) == 0
    assert methods.check_selection("balanced", 4) == 4
    with pytest.raises(ValueError, match="fill"):
        methods.check_selection("global", 0, "policy", "skip", fill="nearest", fill_name="fill")
    with pytest.raises(ValueError, match="seed_frac"):
        methods.check_selection("global", 0, "policy", "skip", fill="kcenter", seed_frac=-1,
                                frac_name="seed_frac")
    with pytest.raises(ValueError, match="skip"):
        methods.check_selection("global", 2, "policy", "skip", fill="kcenter")


def test_config_and_command_line_plumbing(tmp_path):
    assert config.DEFAULTS["select_fill"] == "score"
    assert config.DEFAULTS["kcenter_seed_frac"] == 0.0 and config.DEFAULTS["kcenter_ckpt"] == -1
    (tmp_path / "c.yaml").write_text("dataset: synthetic-cifar10\nbatch_size: 128\n"
                                     "select_fill: kcenter\nkcenter_seed_frac: 0.1\n"
                                     "kcenter_ckpt: 0\nselect_policy: balanced\n")
    cfg = config.load_config(str(tmp_path / "c.yaml"))
    e = score.engine_config(cfg)
    assert (e.select_fill, e.kcenter_seed_frac, e.kcenter_ckpt) == ("kcenter", 0.1, 0)
    assert e.select_policy == "balanced" and not e.default_selection()
    (tmp_path / "d.yaml").write_text("dataset: synthetic-cifar10\nbatch_size: 128\n")
    d = score.engine_config(config.load_config(str(tmp_path / "d.yaml")))
    assert d.select_fill == "score" and d.default_selection()
    assert score.parse(["--fill", "kcenter"]).fill == "kcenter"
    assert score.parse([]).fill is None
    with pytest.raises(SystemExit):
        score.parse(["--fill", "nearest"])
    cfg["select_skip"] = 2  # the combination is rejected where the engine config is built
    with pytest.raises(ValueError, match="select_skip"):
        score.engine_config(cfg)


def test_limits_have_one_owner():
    """The wrapper's limits are the header's defines, and the seed batch a launch folds comes
    from the library (the work estimate and the tests read it there)."""
    import os
    import re
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    src = open(os.path.join(root, "include", "dd_capi.h")).read()
    defs = {k: int(v) for k, v in re.findall(r"#define (DD_KCENTER_\w+) (\d+)", src)}
    assert defs == {"DD_KCENTER_MAX_SEED_BATCH": _capi.KCENTER_MAX_SEED_BATCH,
                    "DD_KCENTER_MAX_BLOCKS": _capi.KCENTER_MAX_BLOCKS,
                    "DD_KCENTER_MAX_GROUPS": _capi.KCENTER_MAX_GROUPS}
    L = _capi.lib()
    assert L.dd_kcenter_seed_batch(512, 0) == 8 and L.dd_kcenter_seed_batch(512, 3) == 3
    assert L.dd_kcenter_seed_batch(512, 64) == 24   # 48 KB of 2 KB centres
    assert L.dd_kcenter_seed_batch(4096, 0) == 3    # 16 KB each
    assert L.dd_kcenter_seed_batch(512, 65) == 0 and L.dd_kcenter_seed_batch(0, 0) == 0
    assert _capi.kcenter_workspace_bytes(300, 512, _capi.KCENTER_MAX_GROUPS + 1, 1) == 0


def test_infinite_radius_is_null_in_the_metadata():
    import json
    from data_diet_distributed_amd.subset_index import json_radius
    assert json.dumps(json_radius([1.5, float("inf"), 0.0])) == "[1.5, null, 0.0]"


def test_entry_points_validate_before_launching():
    """Host only: the workspace query, and bad arguments rejected with a message."""
    L = _capi.lib()
    assert _capi.kcenter_workspace_bytes(50000, 512, 1, 25000) == 25000 * 8 + 192  # to 256
    assert _capi.kcenter_workspace_bytes(300, 17, 4, 0) == 256
    assert _capi.kcenter_workspace_bytes(300, 4097, 1, 10) == 0
    assert _capi.kcenter_workspace_bytes(1 << 31, 512, 1, 10) == 0
    assert _capi.kcenter_workspace_bytes(300, 512, 0, 10) == 0
    assert _capi.kcenter_workspace_bytes(300, 512, 1, 301) == 0
    P16 = ctypes.c_void_p(16)
    args = [P16, P16, 300, 512, P16, 1, P16, P16, 1, P16, 10, 0, 0, P16, P16, P16, P16]
    assert L.dd_kcenter_greedy(*args, None, 0, None) == -1
    assert b"workspace" in L.dd_last_error()
    bad = list(args)
    bad[11] = 65  # seed_batch
    assert L.dd_kcenter_greedy(*bad, P16, 1 << 20, None) == -1
    assert b"seed_batch" in L.dd_last_error()
    bad = list(args)
    bad[0] = None
    assert L.dd_kcenter_greedy(*bad, P16, 1 << 20, None) == -1
    assert b"null rows" in L.dd_last_error()
    assert L.dd_kcenter_greedy(None, None, 0, 512, None, 1, None, None, 0, None, 0, 0, 0, None,
                               None, None, None, None, 0, None) == 0  # n = 0
