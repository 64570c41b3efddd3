"""ScoreConfig.kcenter_objective = "inertia" on the host: the float64 restatement of the greedy
k-medoids fill the device tests compare against, its own checks, and the plumbing."""
import ctypes
import itertools
import math
import os
import re

import numpy as np
import pytest
import torch

from data_diet_distributed_amd import _capi, config, methods, score, scoring
from data_diet_distributed_amd.get_scores_and_prune import sparse_loader
from data_diet_distributed_amd.scoring import ScoreConfig
from test_kcenter_select import ref_kcenter, sq_dists64


def gains64(M, cur):
    """gain_j = sum_i max(cur_i - M[j][i], 0) for every row j (kept rows hold cur = -1)."""
    return np.maximum(cur[None, :] - M, 0.0).sum(axis=1)


def ref_kmedoids(f, ids, groups, seeds, quotas):
    """The inertia fill in float64; ref_kcenter's arguments.  Each pick of a group is its unkept
    row j with the largest gain_j = sum_i max(cur_i - d2(j, i), 0), a tie to the smaller id;
    then cur = min(cur, d2(j, .)).  Returns (picked [steps, G], gain [steps, G], cur [n]): -1
    past a group's picks; cur -1 for a kept row, +inf where the group keeps nothing."""
    f = np.asarray(f, dtype=np.float64)
    ids, groups = np.asarray(ids, dtype=np.int64), np.asarray(groups, dtype=np.int64)
    seeds = np.asarray(seeds, dtype=np.int64)
    G, n = len(quotas), len(f)
    picks = [int(quotas[g]) - int((groups[seeds] == g).sum()) for g in range(G)]
    assert all(p >= 0 for p in picks)
    steps = max(picks) if picks else 0
    picked = np.full((steps, G), -1, dtype=np.int64)
    gain = np.full((steps, G), -1.0)
    out = np.full(n, np.inf)
    for g in range(G):
        member = np.nonzero(groups == g)[0]
        M = sq_dists64(f[member])
        gid = ids[member]
        cur = np.full(len(member), np.inf)
        for c in np.nonzero(np.isin(member, seeds))[0]:
            cur = np.minimum(cur, M[c])
        cur[np.isin(member, seeds)] = -1.0
        for t in range(picks[g]):
            gj = gains64(M, cur)
            gj[cur < 0] = -np.inf  # kept: never a candidate again
            tied = np.nonzero(gj == gj.max())[0]
            c = tied[np.argmin(gid[tied])]
            picked[t, g], gain[t, g] = gid[c], gj[c]
            cur = np.minimum(cur, M[c])
            cur[c] = -1.0
        out[member] = cur
    return picked, gain, out


def inertia(cur):
    return np.maximum(cur, 0.0).sum()


# ---- the restatement's own checks ----------------------------------------------------------
@pytest.mark.parametrize("n,D,k", [(10, 2, 3), (9, 3, 2), (8, 1, 3)])
def test_ref_against_brute_force(n, D, k):
    """Every step takes the single best addition (brute force over the candidates), the inertia
    never grows, and the total decrease is within Nemhauser's 1 - 1/e of the best k-subset's
    (the decrease is monotone submodular in the kept set)."""
    rng = np.random.default_rng(n * 31 + D)
    f = rng.integers(-6, 7, size=(n, D)).astype(np.float32)
    d2 = sq_dists64(f)
    ids, groups = rng.permutation(n), np.zeros(n, int)

    def left(kept):  # the inertia of a kept set
        return np.delete(d2[list(kept)].min(axis=0), list(kept)).sum()

    for seed in range(n):
        picked, gain, cur = ref_kmedoids(f, ids, groups, [seed], [k + 1])
        rows = [int(np.nonzero(ids == p)[0][0]) for p in picked[:, 0]]
        kept, seq = [seed], [left([seed])]
        for t, r in enumerate(rows):
            # the decrease every single addition would bring (integer rows: exact)
            drop = {j: seq[-1] - left(kept + [j]) for j in range(n) if j not in kept}
            assert drop[r] == max(drop.values()) == gain[t, 0], (seed, t)
            assert ids[r] == min(ids[j] for j in drop if drop[j] == drop[r])  # the tie rule
            kept.append(r)
            seq.append(left(kept))
        assert all(a >= b for a, b in zip(seq, seq[1:])) and seq[-1] == inertia(cur)
        others = [j for j in range(n) if j != seed]
        opt = min(left([seed] + list(S)) for S in itertools.combinations(others, k))
        assert seq[0] - seq[-1] >= (1 - 1 / math.e) * (seq[0] - opt) - 1e-9


def test_inertia_takes_the_blobs_where_radius_takes_the_outlier():
    """Two tight well-separated blobs and one outlier farther from both than they are apart, a
    seed in the first blob, quota 2: the inertia pick is a member of the other blob (it brings
    12 rows 100 closer, the outlier only itself 425), farthest-first takes the outlier."""
    rng = np.random.default_rng(8)
    a = rng.normal(0.0, 0.1, size=(12, 2))
    b = rng.normal(0.0, 0.1, size=(12, 2)) + [10.0, 0.0]
    f = np.concatenate([a, b, [[5.0, 20.0]]]).astype(np.float32)
    n = len(f)
    ids, groups = np.arange(n), np.zeros(n, int)
    p_in, _, cur_in = ref_kmedoids(f, ids, groups, [3], [2])
    p_r, _, cur_r = ref_kcenter(f, ids, groups, [3], [2])
    assert 12 <= p_in[0, 0] < 24 and p_r[0, 0] == n - 1
    assert inertia(cur_in) < inertia(cur_r) and cur_in.max() > cur_r.max()


# ---- configuration -------------------------------------------------------------------------
def test_objective_validation_and_plumbing(tmp_path):
    assert methods.KCENTER_OBJECTIVES == ("radius", "inertia")
    assert ScoreConfig().kcenter_objective == config.DEFAULTS["kcenter_objective"] == "radius"
    assert ScoreConfig().default_selection()
    k = ScoreConfig(select_fill="kcenter", kcenter_objective="inertia")
    assert k.kcenter_objective == "inertia" and not k.default_selection()
    for bad in ("medoid", None, 1):
        with pytest.raises(ValueError, match="kcenter_objective"):
            ScoreConfig(kcenter_objective=bad)  # checked whatever the fill
        with pytest.raises(ValueError, match="objective"):
            methods.check_objective(bad, "objective")
    (tmp_path / "c.yaml").write_text("dataset: synthetic-cifar10\nbatch_size: 128\n"
                                     "select_fill: kcenter\nkcenter_objective: inertia\n")
    cfg = config.load_config(str(tmp_path / "c.yaml"))
    assert score.engine_config(cfg).kcenter_objective == "inertia"
    assert score.parse(["--fill-objective", "inertia"]).fill_objective == "inertia"
    assert score.parse([]).fill_objective is None
    with pytest.raises(SystemExit):
        score.parse(["--fill-objective", "sum"])
    cfg["kcenter_objective"] = "sum"
    with pytest.raises(ValueError, match="kcenter_objective"):
        score.engine_config(cfg)


def test_rejections_before_any_launch():
    with pytest.raises(ValueError, match="objective"):
        sparse_loader(None, 10, None, "cpu", 0.5, 8, 0, objective="medoid")
    keys, rows = torch.zeros(8), torch.zeros((8, 2))
    with pytest.raises(ValueError, match="objective"):
        scoring.select_with_policy(keys, None, None, 4, objective="sum")
    n = _capi.KMEDOIDS_MAX_GROUP_ROWS + 1
    with pytest.raises(ValueError, match="stratified"):
        scoring.select_with_policy(torch.zeros(n), None, None, 10, fill="kcenter",
                                   rows=torch.zeros((n, 2)), objective="inertia")


def test_entry_points_validate_before_launching():
    """Host only: the limit's one owner, the workspace query, bad arguments with a message."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    src = open(os.path.join(root, "include", "dd_capi.h")).read()
    assert int(re.search(r"#define DD_KMEDOIDS_MAX_GROUP_ROWS (\d+)", src).group(1)) == \
        _capi.KMEDOIDS_MAX_GROUP_ROWS == 16384
    assert _capi.kmedoids_workspace_bytes(301, 17, [130, 1, 0, 170], 40) > 4 * 300 * 192
    for bad in ((301, 17, [301], 40, "fp32"), (301, 4097, [301], 40), (300, 17, [301], 40),
                (20000, 17, [16385], 4)):
        assert _capi.kmedoids_workspace_bytes(*bad) == 0
    P16, big = ctypes.c_void_p(16), (ctypes.c_int64 * 1)(16385)
    assert _capi.lib().dd_kmedoids_greedy(P16, P16, 20000, 512, P16, big, 1, P16, P16, 1, P16, 10,
                                          1, 0, 0, P16, P16, P16, P16, P16, 1 << 40, None) == -1
    assert b"DD_KMEDOIDS_MAX_GROUP_ROWS" in _capi.lib().dd_last_error()
