"""kcenter_cover = "ball" through the product layers: ScoringEngine.run under "balanced" on the
case of tests/test_gpu_kcenter_engine.py (ResNet-18, K = 3 synthetic checkpoints, N = 300, 10
classes), checked on the rows the run gathered."""
import numpy as np
import pytest
import torch

from data_diet_distributed_amd import methods
from data_diet_distributed_amd.scoring import select_with_policy
from test_gpu_kcenter_engine import C, D, FRAC, case, engine  # noqa: F401 (case: a fixture)
from test_nn_scores import E_OP

pytestmark = pytest.mark.gpu


def test_run_with_the_ball_cover(cuda, case):  # noqa: F811
    img, lab, labels = case["img"], case["lab"], case["labels"]
    eng = engine(case, cuda, select_policy="balanced", kcenter_cover="ball", cover_radius=0.5)
    full, kept, k = eng.run(img, lab, 0.5)
    rec, got = eng.last_selection, kept.cpu().numpy()
    quotas, m = rec["class_quota"], rec["class_seeds"]
    assert k == 150 and len(set(got.tolist())) == k and sum(quotas) == k
    assert np.bincount(labels[got], minlength=C).tolist() == quotas
    assert m == methods.seed_counts(quotas, FRAC) and rec["radius"] is None
    assert rec["cover"] == "ball" and rec["cover_radius"] == 0.5
    seeds = select_with_policy(full["el2n"], lab, C, sum(m), "balanced")[0]
    assert set(seeds.tolist()) == set(got[:sum(m)].tolist())  # the seeds: each class's top m_c
    # theta and the coverage from the rows in float64.  A matrix entry is within E = 2 (eps + 2 u)
    # max ||f||^2 of float64 (the bound tests/test_gpu_herding.py states) and theta within 1e-5 of
    # it, so the covered rows lie between the counts at theta -+ (E + 1e-5 theta).
    rows = eng._kcenter_rows.cpu().numpy().astype(np.float64)
    for c in range(C):
        x, mine = rows[labels == c], rows[got[labels[got] == c]]
        theta = 0.5 * 2.0 * ((x - x.mean(axis=0)) ** 2).sum() / len(x)
        assert rec["theta"][c] == pytest.approx(theta, rel=1e-5)
        near = ((x[:, None, :] - mine[None, :, :]) ** 2).sum(axis=2).min(axis=1)
        E = 2 * (E_OP["f16x3"] + (D + 4) * 2.0 ** -24) * (x ** 2).sum(axis=1).max() + 1e-5 * theta
        lo, hi = ((near <= theta + s * E).sum() for s in (-1, 1))
        assert lo <= round(rec["coverage"][c] * len(x)) <= hi and 0 < lo
    other = engine(case, cuda, select_policy="balanced", kcenter_cover="ball", cover_radius=0.5,
                   el2n_chunk=256)
    assert torch.equal(other.run(img, lab, 0.5)[1], kept) and other.last_selection == rec


def test_cover_none_is_the_plain_fill(cuda, case):  # noqa: F811
    img, lab = case["img"], case["lab"]
    plain = engine(case, cuda, select_policy="balanced")
    named = engine(case, cuda, select_policy="balanced", kcenter_cover="none", cover_radius=0.7)
    a, b = plain.run(img, lab, 0.5)[1], named.run(img, lab, 0.5)[1]
    assert torch.equal(a, b) and named.last_selection == plain.last_selection
    assert not {"cover", "cover_radius", "theta", "coverage"} & set(named.last_selection)
