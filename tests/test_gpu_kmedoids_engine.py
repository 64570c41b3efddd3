"""The inertia objective of the kcenter fill through the product layers: ScoringEngine.run under
"stratified" on the case of tests/test_gpu_kcenter_engine.py (ResNet-18, K = 3 synthetic
checkpoints, N = 300, 10 classes), against select_with_policy on the rows the run gathered."""
import numpy as np
import pytest
import torch

from data_diet_distributed_amd.scoring import apportion, select_with_policy
from test_gpu_kcenter_engine import C, FRAC, N, case, engine  # noqa: F401 (case: a fixture)

pytestmark = pytest.mark.gpu


def test_run_with_the_inertia_objective(cuda, case):  # noqa: F811
    img, lab = case["img"], case["lab"]
    eng = engine(case, cuda, select_policy="stratified", kcenter_objective="inertia")
    full, kept, k = eng.run(img, lab, 0.5)
    rec = eng.last_selection
    quotas = apportion(k, np.bincount(case["labels"], minlength=C).tolist(), "stratified")
    got = kept.cpu().numpy()
    assert k == 150 and len(set(got.tolist())) == k and rec["class_quota"] == quotas
    assert np.bincount(case["labels"][got], minlength=C).tolist() == quotas
    assert rec["objective"] == "inertia" and len(rec["inertia"]) == C == len(rec["radius"])
    assert all(np.isfinite(v) and v > 0 for v in rec["inertia"])
    # the standalone selection on the gathered rows
    alone, rec2 = select_with_policy(full["el2n"], lab, C, k, "stratified", fill="kcenter",
                                     seed_frac=FRAC, rows=eng._kcenter_rows,
                                     objective="inertia")
    assert torch.equal(alone, kept) and rec2 == rec
    other = engine(case, cuda, select_policy="stratified", kcenter_objective="inertia",
                   el2n_chunk=256)
    assert torch.equal(other.run(img, lab, 0.5)[1], kept) and other.last_selection == rec
    # "radius" is today's fill, bit for bit, and another keep-set than "inertia"
    plain = engine(case, cuda, select_policy="stratified")
    named = engine(case, cuda, select_policy="stratified", kcenter_objective="radius")
    a, b = plain.run(img, lab, 0.5)[1], named.run(img, lab, 0.5)[1]
    assert torch.equal(a, b) and named.last_selection == plain.last_selection
    assert not {"objective", "inertia"} & set(named.last_selection)
    assert not torch.equal(a, kept) and torch.equal(a[:sum(rec["class_seeds"])],
                                                    kept[:sum(rec["class_seeds"])])
