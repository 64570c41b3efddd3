"""The d2 diversity through the product layers: select_with_policy and ScoringEngine.run on the case
of tests/test_gpu_kcenter_engine.py (ResNet-18, K = 3 synthetic checkpoints, N = 300, 10 classes),
against the NumPy restatement of tests/test_d2_select.py fed the engine's own scores and the graph
dd_knn returns for the engine's rows (the weights are dd_d2_weights', checked on their own in
tests/test_gpu_d2.py)."""
import numpy as np
import pytest
import torch

from data_diet_distributed_amd import _capi
from data_diet_distributed_amd.scoring import ScoreConfig, ScoringEngine, select_with_policy
from test_d2_select import ref_propagate, ref_select
from test_gpu_kcenter_engine import C, N, case  # noqa: F401 (case: a fixture)

pytestmark = pytest.mark.gpu

D2K, GF, GR = 6, 1.0, 2.0


def engine(case, cuda, **kw):
    kw.setdefault("el2n_chunk", 128)
    kw.setdefault("select_diversity", "d2")
    return ScoringEngine(case["models"], ScoreConfig(d2_k=D2K, d2_gamma_f=GF, d2_gamma_r=GR, **kw),
                         cuda)


def restatement(keys, rows, labels, quotas, scale):
    """kept by the float32 loops, from the graph of `rows` and the recorded scale."""
    n = keys.numel()
    ids = torch.arange(n, device=keys.device)
    dist = torch.empty((n, D2K), dtype=torch.float32, device=keys.device)
    nbr = torch.empty((n, D2K), dtype=torch.int64, device=keys.device)
    _capi.knn(rows, ids, rows, ids, D2K, dist=dist, nbr_id=nbr)
    sq = dist.cpu().numpy().astype(np.float64) ** 2
    # (two float64 sums of n k positive terms: each within n k 2^-53 of the mean)
    assert np.isfinite(sq).all() and abs(scale / sq.mean() - 1) <= 2 * sq.size * 2.0 ** -53
    w_f, w_r = (_capi.d2_weights(dist, nbr, float(np.float32(g / scale))).cpu().numpy()
                for g in (GF, GR))
    x1 = ref_propagate(keys.cpu().numpy(), nbr.cpu().numpy(), w_f, np.float32)
    return ref_select(x1, nbr.cpu().numpy(), w_r, labels, quotas, np.float32)[0]


@pytest.mark.parametrize("policy", ["global", "balanced"])
def test_run_with_the_d2_diversity(cuda, case, policy):  # noqa: F811
    img, lab = case["img"], case["lab"]
    eng = engine(case, cuda, select_policy=policy)
    full, kept, k = eng.run(img, lab, 0.5)
    rec = eng.last_selection
    assert k == 150 and eng.last_refine is None
    assert [rec[key] for key in ("diversity", "d2_k", "d2_gamma_f", "d2_gamma_r")] == [
        "d2", D2K, GF, GR]
    labels, quotas = (None, [k]) if policy == "global" else (case["labels"], rec["class_quota"])
    want = restatement(full["el2n"], eng._kcenter_rows, labels, quotas, rec["d2_scale"])
    assert np.array_equal(kept.cpu().numpy(), want) and len(set(want.tolist())) == k
    plain = engine(case, cuda, select_policy=policy, select_diversity="none")
    assert not torch.equal(plain.run(img, lab, 0.5)[1], kept)  # (the option is not ignored)
    # the geometry of the scoring: another chunk size, the n_total mode, and two shards scored
    # one after the other whose scores and rows are put together by hand
    for other, kw in ((engine(case, cuda, select_policy=policy, el2n_chunk=256), {}),
                      (engine(case, cuda, select_policy=policy), {"n_total": N})):
        assert torch.equal(other.run(img, lab, 0.5, **kw)[1], kept), (policy, kw)
        assert other.last_selection == rec
    keys, rows = [], []
    for lo, hi in ((0, 128), (128, N)):
        keys.append(eng.score_shard(img, lab, lo, hi)["el2n"])
        rows.append(eng._kcenter_rows.clone())
    alone, rec2 = select_with_policy(torch.cat(keys), lab, C, k, policy, diversity="d2", d2_k=D2K,
                                     gamma_f=GF, gamma_r=GR, rows=torch.cat(rows))
    assert torch.equal(alone, kept) and rec2 == rec


@pytest.mark.parametrize("policy", ["global", "stratified"])
def test_zero_weights_give_the_score_fill(cuda, policy):
    """With gammas so large that every weight underflows to 0 nothing is absorbed and nothing is
    sent: the selection is the rank cut, order included (no two rows coincide, so no distance is
    0 and no weight stays 1)."""
    g = torch.Generator().manual_seed(3)
    rows = torch.randn((400, 24), generator=g).to(cuda)
    keys = torch.rand(400, generator=g).to(cuda)
    labels = torch.randint(0, 4, (400,), generator=g).to(cuda)
    assert len(torch.unique(rows, dim=0)) == 400
    cut, rec = select_with_policy(keys, labels, 4, 150, policy)
    kept, rec2 = select_with_policy(keys, labels, 4, 150, policy, diversity="d2", d2_k=5,
                                    gamma_f=1e6, gamma_r=1e6, rows=rows)
    assert rec2["d2_scale"] > 0 and {k: rec2[k] for k in rec} == rec
    if policy == "global":
        assert torch.equal(kept, cut)
    else:  # the class cut orders by class; D2 picks by score: the same rows per class, in order
        for c in range(4):
            assert torch.equal(kept[labels[kept] == c], cut[labels[cut] == c])
        assert torch.equal(keys[kept], keys[kept].sort(descending=True)[0])


def test_no_diversity_is_todays_selection(cuda, case):  # noqa: F811
    img, lab = case["img"], case["lab"]
    plain = ScoringEngine(case["models"], ScoreConfig(el2n_chunk=128, select_policy="balanced"),
                          cuda)
    named = engine(case, cuda, select_policy="balanced", select_diversity="none")
    a, b = plain.run(img, lab, 0.5), named.run(img, lab, 0.5)
    assert a[2] == b[2] and torch.equal(a[1], b[1]) and torch.equal(a[0]["el2n"], b[0]["el2n"])
    assert named.last_selection == plain.last_selection
    assert set(named.last_selection) == {"policy", "skip", "class_counts", "class_skip",
                                         "class_quota"}
    assert named._kcenter_rows is None  # no rows are kept without a row-based selection
