"""ScoreConfig.kcenter_match = "mean" on the host: the float64 restatement of kernel herding the
device tests compare against, the plumbing and the entry points' rejections."""
import ctypes

import numpy as np
import pytest
import torch

from data_diet_distributed_amd import _capi, config, methods, score, scoring
from data_diet_distributed_amd.get_scores_and_prune import sparse_loader
from data_diet_distributed_amd.scoring import ScoreConfig


def herding_values(f, kept):
    """v_i = A_i - (t + 1) P_i of every row of one group f [n, D] (float64) with the rows `kept`
    (t of them): A_i the sum of squared distances from the kept rows to row i, P_i row i's to
    the group mean; -inf for a kept row."""
    f = np.asarray(f, dtype=np.float64)
    sq = (f ** 2).sum(axis=1)
    A = (sq[kept][:, None] + sq[None, :] - 2.0 * f[kept] @ f.T).sum(axis=0)
    v = A - (len(kept) + 1) * ((f - f.mean(axis=0)) ** 2).sum(axis=1)
    v[kept] = -np.inf
    return v


def ref_herding(f, ids, groups, seeds, quotas):
    """The herding fill in float64: group g folds its seeds (indices of rows of f), then takes
    quotas[g] - (its seeds) picks, each its unkept row with the largest v, a tie to the smaller
    id.  Returns (picked [steps, G], value [steps, G]), -1 past a group's picks."""
    ids, groups, seeds = (np.asarray(a, dtype=np.int64) for a in (ids, groups, seeds))
    G = len(quotas)
    picks = [int(quotas[g]) - int((groups[seeds] == g).sum()) for g in range(G)]
    picked = np.full((max(picks), G), -1, dtype=np.int64)
    value = np.full((max(picks), G), -1.0)
    for g in range(G):
        member = np.nonzero(groups == g)[0]
        kept = [int(np.nonzero(member == s)[0][0]) for s in seeds[groups[seeds] == g]]
        for t in range(picks[g]):
            v = herding_values(f[member], kept)
            tied = np.nonzero(v == v.max())[0]
            c = int(tied[np.argmin(ids[member][tied])])
            picked[t, g], value[t, g] = ids[member][c], v[c]
            kept.append(c)
    return picked, value


def test_match_validation_and_plumbing(tmp_path):
    assert methods.KCENTER_MATCH == ("none", "mean")
    assert ScoreConfig().kcenter_match == config.DEFAULTS["kcenter_match"] == "none"
    assert ScoreConfig().default_selection()
    k = ScoreConfig(select_fill="kcenter", kcenter_match="mean")
    assert k.kcenter_match == "mean" and not k.default_selection()
    for kw, name in (({"kcenter_match": "median"}, "kcenter_match"),
                     ({"kcenter_match": "mean"}, "select_fill"),
                     ({"kcenter_match": "mean", "select_fill": "kcenter",
                       "kcenter_objective": "inertia"}, "kcenter_objective")):
        with pytest.raises(ValueError, match=name):
            ScoreConfig(**kw)
    assert methods.check_match("none", "score", "inertia") == "none"
    with pytest.raises(ValueError, match="objective"):
        methods.check_match("mean", "kcenter", "inertia", objective_name="objective")
    (tmp_path / "c.yaml").write_text("dataset: synthetic-cifar10\nbatch_size: 128\n"
                                     "select_fill: kcenter\nkcenter_match: mean\n")
    cfg = config.load_config(str(tmp_path / "c.yaml"))
    assert score.engine_config(cfg).kcenter_match == "mean"
    args = score.parse(["--fill-match", "none"])
    assert args.fill_match == "none" and score.parse([]).fill_match is None
    assert score.engine_config(score.apply_overrides(cfg, args)).kcenter_match == "none"
    with pytest.raises(SystemExit):
        score.parse(["--fill-match", "median"])


def test_rejections_before_any_launch():
    with pytest.raises(ValueError, match="match"):
        sparse_loader(None, 10, None, "cpu", 0.5, 8, 0, fill="kcenter", match="median")
    with pytest.raises(ValueError, match="fill"):
        scoring.select_with_policy(torch.zeros(8), None, None, 4, match="mean")
    n = _capi.KMEDOIDS_MAX_GROUP_ROWS + 1
    with pytest.raises(ValueError, match="stratified"):
        scoring.select_with_policy(torch.zeros(n), None, None, 10, fill="kcenter",
                                   rows=torch.zeros((n, 2)), match="mean")


def test_entry_points_validate_before_launching():
    """Host only: the symbols, the ABI, the workspace query, bad arguments with a message."""
    assert {"dd_herding_workspace_bytes", "dd_herding_greedy"} <= set(_capi.EXPORTS)
    lib = _capi.lib()
    assert lib.dd_abi_version() == 10
    need = _capi.herding_workspace_bytes(301, 17, [130, 1, 0, 170], 40)
    assert need > 4 * (130 * 192 + 170 * 192) + 4 * 12 * 17
    for bad in ((301, 17, [301], 40, "fp32"), (301, 4097, [301], 40), (300, 17, [301], 40),
                (20000, 17, [16385], 4)):
        assert _capi.herding_workspace_bytes(*bad) == 0
    P16, sizes = ctypes.c_void_p(16), (ctypes.c_int64 * 1)(301)
    need = _capi.herding_workspace_bytes(301, 17, [301], 10)

    def call(n=301, sizes=sizes, rows=P16, picked=P16, ws=P16, ws_bytes=1 << 40):
        return lib.dd_herding_greedy(rows, P16, n, 17, P16, sizes, 1, P16, P16, 1, P16, 10, 1, 0,
                                     picked, P16, P16, ws, ws_bytes, None)

    for kw, msg in (({"n": 20000, "sizes": (ctypes.c_int64 * 1)(16385)},
                     b"DD_KMEDOIDS_MAX_GROUP_ROWS"), ({"rows": None}, b"null rows"),
                    ({"picked": None}, b"null picked"), ({"ws": None}, b"workspace"),
                    ({"ws_bytes": need - 1}, b"dd_herding_workspace_bytes")):
        assert call(**kw) == -1 and msg in lib.dd_last_error(), kw
