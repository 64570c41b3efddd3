"""The d2 diversity on the host: the new fields' validation, the config and command-line plumbing,
the entry points' argument checks, and the NumPy restatement of include/dd_capi.h's dd_d2_propagate
and dd_d2_select that the GPU tests compare the kernels with."""
import ctypes

import numpy as np
import pytest

from data_diet_distributed_amd import _capi, config, methods, score
from data_diet_distributed_amd.scoring import ScoreConfig, ScoringEngine


def ref_propagate(x0, nbr, w, dt):
    """x1[i] = x0[i] + sum_j w[i][j] x0[nbr[i][j]] over the used slots in ascending order, every
    product and sum rounded to `dt`."""
    x0 = x0.astype(dt)
    x1 = x0.copy()
    for i in range(len(x0)):
        for j in range(nbr.shape[1]):
            if nbr[i, j] >= 0:
                x1[i] = dt(x1[i] + dt(dt(w[i, j]) * x0[nbr[i, j]]))
    return x1


def ref_select(x, nbr, w, group, quota, dt, exact=False):
    """The header's loop in `dt`.  Returns (picked, value, messages skipped because their target
    was retired); with `exact` every updated score must be a float32, so that the float64 loop is
    also what correctly rounded fp32 arithmetic gives."""
    x, quota = x.astype(dt).copy(), list(quota)
    live = np.ones(len(x), dtype=bool)
    total, picked, value, skipped = sum(quota), [], [], 0
    while len(picked) < total and live.any():
        s = int(np.argmax(np.where(live, x, -np.inf)))  # (the first of equal maxima)
        live[s] = False
        g = 0 if group is None else int(group[s])
        if quota[g] == 0:
            continue
        picked.append(s)
        value.append(x[s])
        quota[g] -= 1
        for j in range(nbr.shape[1]):
            v = nbr[s, j]
            skipped += v >= 0 and not live[v]
            if v >= 0 and live[v]:
                x[v] = dt(x[v] - dt(dt(w[s, j]) * x[s]))
                assert not exact or np.float32(x[v]) == x[v]
    tail = total - len(picked)
    return (np.array(picked + [-1] * tail, dtype=np.int64),
            np.array(value + [-1.0] * tail, dtype=dt), skipped)


def test_the_diversity_tuple_and_its_check():
    assert methods.SELECT_DIVERSITY == ("none", "d2")
    assert methods.check_diversity("d2", 16, 0, 2.5) == (16, 0.0, 2.5)
    assert methods.check_diversity("none", np.int64(1), 1, 1, fill="kcenter", skip=3) == (1, 1., 1.)
    with pytest.raises(ValueError, match="select_diversity"):
        methods.check_diversity("dpp")
    for bad in (0, 17, 2.0, True, "4"):
        with pytest.raises(ValueError, match="d2_k"):
            methods.check_diversity("none", bad)
    for bad in (-0.5, float("inf"), float("nan"), "1", True):
        with pytest.raises(ValueError, match="d2_gamma_f"):
            methods.check_diversity("d2", 10, bad, 1.0)
        with pytest.raises(ValueError, match="gr"):
            methods.check_diversity("none", 10, 1.0, bad, gamma_r_name="gr")
    with pytest.raises(ValueError, match="select_fill"):
        methods.check_diversity("d2", fill="kcenter")
    with pytest.raises(ValueError, match="select_skip"):
        methods.check_diversity("d2", skip=2)


def test_score_config_fields():
    d = ScoreConfig()
    assert (d.select_diversity, d.d2_k, d.d2_gamma_f, d.d2_gamma_r) == ("none", 10, 1.0, 1.0)
    assert d.default_selection() and d.row_selection() is None
    c = ScoreConfig(select_diversity="d2", d2_k=4, d2_gamma_f=0, select_policy="balanced")
    assert not c.default_selection() and c.refine == "auto" and c.d2_gamma_f == 0.0
    assert not ScoreConfig(select_diversity="d2").default_selection()
    for kw, name in (({"select_diversity": "graph"}, "select_diversity"), ({"d2_k": 17}, "d2_k"),
                     ({"d2_gamma_f": -1}, "d2_gamma_f"), ({"d2_gamma_r": float("nan")}, "d2_gamma_r"),
                     ({"select_diversity": "d2", "select_fill": "kcenter"}, "select_fill"),
                     ({"select_diversity": "d2", "select_skip": 1}, "select_skip"),
                     ({"select_diversity": "d2", "refine": True}, "refine=True")):
        with pytest.raises(ValueError, match=name):  # (the numbers: whatever the diversity)
            ScoreConfig(**kw)
    with pytest.raises(ValueError, match="kcenter_ckpt"):  # (before anything looks at the models)
        ScoringEngine([object()] * 3, ScoreConfig(select_diversity="d2", kcenter_ckpt=3), "cuda:0")


def test_config_and_command_line_round_trip(tmp_path):
    assert [config.DEFAULTS[k] for k in ("select_diversity", "d2_k", "d2_gamma_f",
                                         "d2_gamma_r")] == ["none", 10, 1.0, 1.0]
    (tmp_path / "c.yaml").write_text("dataset: synthetic-cifar10\nbatch_size: 128\n"
                                     "select_diversity: d2\nd2_k: 6\nd2_gamma_r: 0.5\n")
    cfg = config.load_config(str(tmp_path / "c.yaml"))
    e = score.engine_config(cfg)
    assert (e.select_diversity, e.d2_k, e.d2_gamma_f, e.d2_gamma_r) == ("d2", 6, 1.0, 0.5)
    args = score.parse(["--diversity", "none", "--d2-k", "3", "--d2-gamma-f", "2",
                        "--d2-gamma-r", "0"])
    e = score.engine_config(score.apply_overrides(cfg, args))
    assert (e.select_diversity, e.d2_k, e.d2_gamma_f, e.d2_gamma_r) == ("none", 3, 2.0, 0.0)
    assert score.parse([]).diversity is None
    with pytest.raises(SystemExit):
        score.parse(["--diversity", "dpp"])
    with pytest.raises(ValueError, match="d2_k"):
        score.engine_config(dict(cfg, d2_k=0))


def test_entry_points_validate_before_launching():
    """Host only: the limits, the workspace query, and bad arguments rejected with a message."""
    L, P16 = _capi.lib(), ctypes.c_void_p(16)
    assert (_capi.D2_MAX_ROWS, _capi.D2_MAX_GROUPS) == (1 << 21, 16384)
    assert _capi.d2_workspace_bytes(50000, 10) == 196 * 1024 + 1024  # 196 blocks, their maxima
    assert _capi.d2_workspace_bytes(1 << 21, 16384) == (1 << 23) + (1 << 15)
    assert _capi.d2_workspace_bytes((1 << 21) + 1) == 0 == _capi.d2_workspace_bytes(10, 16385)
    sel = [P16, P16, P16, None, P16, 300, 10, 1, 100, P16, P16, P16]
    assert L.dd_d2_select(*sel, None, 0, None) == -1 and b"workspace" in L.dd_last_error()
    for at, v, word in ((6, 17, b"1 <= k"), (8, 301, b"total"), (7, 2, b"group"), (0, None, b"null x")):
        bad = sel[:at] + [v] + sel[at + 1:]
        assert L.dd_d2_select(*bad, P16, 1 << 20, None) == -1 and word in L.dd_last_error()
    assert L.dd_d2_weights(P16, P16, 300, 10, -1.0, P16, None) == -1
    assert b"coef" in L.dd_last_error()
    assert L.dd_d2_propagate(P16, P16, P16, 300, 4, P16, P16, None) == -1
    assert b"x1 must not be x0" in L.dd_last_error()
