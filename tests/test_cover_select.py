"""ScoreConfig.kcenter_cover = "ball" on the host: the float64 restatement of the ball-cover rule
the device tests compare against, the plumbing and the entry points' rejections."""
import ctypes

import numpy as np
import pytest
import torch

from data_diet_distributed_amd import _capi, config, methods, score, scoring
from data_diet_distributed_amd.get_scores_and_prune import sparse_loader
from data_diet_distributed_amd.scoring import ScoreConfig


def ref_cover(f, ids, groups, seeds, quotas, prio, radius):
    """The cover fill in float64: group g covers its seeds (indices of rows of f), then takes
    quotas[g] - (its seeds) picks, each its unkept valid row whose ball holds the most uncovered
    rows, a tie to the smaller prio.  Returns (picked [steps, G], gain [steps, G], theta [G],
    covered [G], margin): -1 past a group's picks; margin is the smallest |M - theta| / theta over
    the off-diagonal matrix entries of the valid rows."""
    ids, groups, seeds, prio = (np.asarray(a, dtype=np.int64) for a in (ids, groups, seeds, prio))
    G = len(quotas)
    picks = [int(quotas[g]) - int((groups[seeds] == g).sum()) for g in range(G)]
    picked, gain = (np.full((max(picks), G), -1, dtype=np.int64) for _ in range(2))
    theta, covered, margin = np.zeros(G), np.zeros(G, dtype=np.int64), np.inf
    for g in range(G):
        member = np.nonzero(groups == g)[0]
        if not len(member):
            continue
        x, n = f[member].astype(np.float64), len(member)
        valid = np.all(np.abs(x) < 2.0 ** 15, axis=1)  # (a NaN fails it)
        x[~valid] = 0.0
        P = ((x - x.sum(axis=0) / n) ** 2).sum(axis=1)
        theta[g] = radius * (2.0 / n) * P[valid].sum()
        sq = (x ** 2).sum(axis=1)
        M = sq[:, None] + sq[None, :] - 2.0 * x @ x.T
        pair = valid[:, None] & valid[None, :]
        off = pair & ~np.eye(n, dtype=bool)
        if off.any():
            margin = min(margin, np.abs(M[off] / theta[g] - 1.0).min())
        adj = ((M <= theta[g]) | np.eye(n, dtype=bool)) & pair
        unc, kept = valid.copy(), np.isin(member, seeds)
        for j in np.nonzero(kept)[0]:
            unc &= ~adj[j]
        for t in range(picks[g]):
            cand = np.nonzero(valid & ~kept)[0]
            if not len(cand):
                break
            deg = (adj[cand] & unc).sum(axis=1)
            k = np.lexsort((prio[member][cand], -deg))[0]
            picked[t, g], gain[t, g] = ids[member][cand[k]], deg[k]
            unc &= ~adj[cand[k]]
            kept[cand[k]] = True
        covered[g] = (valid & ~unc).sum()
    return picked, gain, theta, covered, margin


def test_the_reference_on_a_line():
    """Five points on a line with mean 0 and sum of squares 122, theta = 2: the middle of the dense
    triple goes first, then the two lone points by prio."""
    f = np.array([[0.0], [1.0], [2.0], [6.0], [-9.0]])
    picked, gain, theta, covered, margin = ref_cover(f, np.arange(5), np.zeros(5, int), [], [3],
                                                     [4, 3, 2, 1, 0], 2.0 / (0.4 * 122))
    assert theta[0] == pytest.approx(2.0) and margin == pytest.approx(0.5)
    assert picked[:, 0].tolist() == [1, 4, 3] and gain[:, 0].tolist() == [3, 1, 1]
    assert covered[0] == 5


def test_cover_validation_and_plumbing(tmp_path):
    assert methods.KCENTER_COVER == ("none", "ball")
    assert ScoreConfig().kcenter_cover == config.DEFAULTS["kcenter_cover"] == "none"
    assert ScoreConfig().cover_radius == config.DEFAULTS["cover_radius"] == 0.25
    assert ScoreConfig().default_selection()
    k = ScoreConfig(select_fill="kcenter", kcenter_cover="ball", cover_radius=1)
    assert k.kcenter_cover == "ball" and k.cover_radius == 1.0 and not k.default_selection()
    for kw, name in (({"kcenter_cover": "cube"}, "kcenter_cover"),
                     ({"cover_radius": 0.0}, "cover_radius"),
                     ({"cover_radius": float("nan")}, "cover_radius"),
                     ({"kcenter_cover": "ball"}, "select_fill"),
                     ({"kcenter_cover": "ball", "select_fill": "kcenter",
                       "kcenter_objective": "inertia"}, "kcenter_objective"),
                     ({"kcenter_cover": "ball", "select_fill": "kcenter",
                       "kcenter_match": "mean"}, "kcenter_match")):
        with pytest.raises(ValueError, match=name):
            ScoreConfig(**kw)
    assert methods.check_cover("none", 2, "score", "inertia", "none") == ("none", 2.0)
    with pytest.raises(ValueError, match="objective"):
        methods.check_cover("ball", 0.25, "kcenter", "inertia", objective_name="objective")
    (tmp_path / "c.yaml").write_text("dataset: synthetic-cifar10\nbatch_size: 128\n"
                                     "select_fill: kcenter\nkcenter_cover: ball\n"
                                     "cover_radius: 0.5\n")
    cfg = config.load_config(str(tmp_path / "c.yaml"))
    ecfg = score.engine_config(cfg)
    assert ecfg.kcenter_cover == "ball" and ecfg.cover_radius == 0.5
    args = score.parse(["--fill-cover", "none", "--cover-radius", "0.125"])
    assert args.fill_cover == "none" and score.parse([]).fill_cover is None
    ecfg = score.engine_config(score.apply_overrides(cfg, args))
    assert ecfg.kcenter_cover == "none" and ecfg.cover_radius == 0.125
    with pytest.raises(SystemExit):
        score.parse(["--fill-cover", "cube"])


def test_rejections_before_any_launch():
    with pytest.raises(ValueError, match="cover"):
        sparse_loader(None, 10, None, "cpu", 0.5, 8, 0, fill="kcenter", cover="cube")
    with pytest.raises(ValueError, match="cover_radius"):
        sparse_loader(None, 10, None, "cpu", 0.5, 8, 0, cover_radius=-1.0)
    with pytest.raises(ValueError, match="fill"):
        scoring.select_with_policy(torch.zeros(8), None, None, 4, cover="ball")
    n = _capi.KMEDOIDS_MAX_GROUP_ROWS + 1
    with pytest.raises(ValueError, match="stratified"):
        scoring.select_with_policy(torch.zeros(n), None, None, 10, fill="kcenter",
                                   rows=torch.zeros((n, 2)), cover="ball")


def test_entry_points_validate_before_launching():
    """Host only: the symbols, the ABI, the workspace query, bad arguments with a message."""
    assert {"dd_cover_workspace_bytes", "dd_cover_greedy"} <= set(_capi.EXPORTS)
    lib = _capi.lib()
    assert lib.dd_abi_version() == 10
    sizes = [130, 1, 0, 170]
    need = _capi.cover_workspace_bytes(301, 17, sizes, 40)
    # herding's workspace, theta, and one bit per float of the matrices (regions of 256 bytes)
    assert need == (_capi.herding_workspace_bytes(301, 17, sizes, 40) + 256
                    + -(-(130 * 192 + 64 + 170 * 192) // 8 // 256) * 256)
    for bad in ((301, 17, [301], 40, "fp32"), (301, 4097, [301], 40), (300, 17, [301], 40),
                (20000, 17, [16385], 4)):
        assert _capi.cover_workspace_bytes(*bad) == 0
    P16, sizes = ctypes.c_void_p(16), (ctypes.c_int64 * 1)(301)
    need = _capi.cover_workspace_bytes(301, 17, [301], 10)

    def call(n=301, sizes=sizes, rows=P16, radius=0.25, prio=P16, picked=P16, ws=P16,
             ws_bytes=1 << 40):
        return lib.dd_cover_greedy(rows, P16, n, 17, P16, sizes, 1, P16, P16, 1, P16, 10, 1, 0,
                                   radius, prio, picked, P16, P16, P16, P16, ws, ws_bytes, None)

    for kw, msg in (({"n": 20000, "sizes": (ctypes.c_int64 * 1)(16385)},
                     b"DD_KMEDOIDS_MAX_GROUP_ROWS"), ({"rows": None}, b"null rows"),
                    ({"prio": None}, b"null rows"), ({"picked": None}, b"null picked"),
                    ({"radius": 0.0}, b"cover_radius"), ({"radius": float("inf")}, b"cover_radius"),
                    ({"ws": None}, b"workspace"),
                    ({"ws_bytes": need - 1}, b"dd_cover_workspace_bytes")):
        assert call(**kw) == -1 and msg in lib.dd_last_error(), kw
