"""kcenter_match = "mean" through the product layers: ScoringEngine.run under "balanced" on the
case of tests/test_gpu_kcenter_engine.py (ResNet-18, K = 3 synthetic checkpoints, N = 300, 10
classes), checked on the rows the run gathered."""
import numpy as np
import pytest
import torch

from data_diet_distributed_amd import methods
from data_diet_distributed_amd.scoring import select_with_policy
from test_gpu_kcenter_engine import C, FRAC, case, engine  # noqa: F401 (case: a fixture)
from test_herding_select import ref_herding

pytestmark = pytest.mark.gpu


def mean_gaps(rows, labels, kept):
    """per class || mean(class) - mean(its kept rows) ||_2 in float64"""
    return [float(np.linalg.norm(rows[labels == c].mean(axis=0)
                                 - rows[kept[labels[kept] == c]].mean(axis=0))) for c in range(C)]


def test_run_with_the_mean_match(cuda, case):  # noqa: F811
    img, lab, labels = case["img"], case["lab"], case["labels"]
    eng = engine(case, cuda, select_policy="balanced", kcenter_match="mean")
    full, kept, k = eng.run(img, lab, 0.5)
    rec, got = eng.last_selection, kept.cpu().numpy()
    quotas, m = rec["class_quota"], rec["class_seeds"]
    assert k == 150 and len(set(got.tolist())) == k and sum(quotas) == k
    assert np.bincount(labels[got], minlength=C).tolist() == quotas
    assert m == methods.seed_counts(quotas, FRAC) and rec["match"] == "mean"
    seeds = select_with_policy(full["el2n"], lab, C, sum(m), "balanced")[0]
    assert set(seeds.tolist()) == set(got[:sum(m)].tolist())  # the seeds: each class's top m_c
    rows = eng._kcenter_rows.cpu().numpy().astype(np.float64)
    gaps = mean_gaps(rows, labels, got)
    assert np.allclose(rec["mean_gap"], gaps, rtol=1e-9, atol=0) and rec["radius"] is None
    # against the rank cut with the same quotas: the device's keep-set and float64's own
    cut = select_with_policy(full["el2n"], lab, C, k, "balanced")[0].cpu().numpy()
    ref = ref_herding(rows, np.arange(len(rows)), labels, got[:sum(m)], quotas)[0]
    for ours in (gaps, mean_gaps(rows, labels, np.concatenate([got[:sum(m)], ref[ref >= 0]]))):
        assert all(a <= b for a, b in zip(ours, mean_gaps(rows, labels, cut)))
    other = engine(case, cuda, select_policy="balanced", kcenter_match="mean", el2n_chunk=256)
    assert torch.equal(other.run(img, lab, 0.5)[1], kept) and other.last_selection == rec


def test_match_none_is_the_plain_fill(cuda, case):  # noqa: F811
    img, lab = case["img"], case["lab"]
    plain = engine(case, cuda, select_policy="balanced")
    named = engine(case, cuda, select_policy="balanced", kcenter_match="none")
    a, b = plain.run(img, lab, 0.5)[1], named.run(img, lab, 0.5)[1]
    assert torch.equal(a, b) and named.last_selection == plain.last_selection
    assert not {"match", "mean_gap"} & set(named.last_selection)
