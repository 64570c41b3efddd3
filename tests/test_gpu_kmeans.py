"""dd_kmeans_assign / dd_kmeans_centroids / forward_scores.kmeans against float64 NumPy: the
header's pick bound and the value bound (both derived in tests/test_nn_scores.py), exact sums."""
import numpy as np
import pytest
import torch

from data_diet_distributed_amd import _capi, forward_scores
from test_nn_scores import E_OP, value_bound

pytestmark = pytest.mark.gpu


def run_assign(dev, f, mu, operands="f16x3", split=None):
    """One call over f, or two accumulating calls over f[:split] and f[split:], as NumPy."""
    n, (Kc, D) = len(f), mu.shape
    mu_d = torch.from_numpy(mu).to(dev)
    sums, counts, bad = (torch.zeros(s, dtype=torch.int64, device=dev) for s in ((Kc, D), Kc, 1))
    assign = torch.full((n,), -7, dtype=torch.int32, device=dev)
    dist = torch.full((n,), -7.0, dtype=torch.float32, device=dev)
    for lo, hi in ((0, n),) if split is None else ((0, split), (split, n)):
        _capi.kmeans_assign(torch.from_numpy(f[lo:hi]).to(dev), mu_d, operands=operands,
                            sums=sums, counts=counts, bad=bad, assign=assign[lo:hi],
                            dist=dist[lo:hi])
    torch.cuda.synchronize()
    return tuple(t.cpu().numpy() for t in (assign, dist, sums, counts, bad))


def d2_all(f, mu):
    """float64 [n, Kc]: the squared distances, from the differences."""
    f, mu = f.astype(np.float64), mu.astype(np.float64)
    return np.stack([((f - m) ** 2).sum(axis=1) for m in mu], axis=1)


def grouped(f, assign, Kc):
    """(int64 [Kc, D] sums of round(v 2^24) over each cluster's rows, int64 [Kc] counts)."""
    live = assign >= 0
    q = np.rint(f[live].astype(np.float64) * 2.0 ** 24).astype(np.int64)
    sums = np.zeros((Kc, f.shape[1]), np.int64)
    np.add.at(sums, assign[live], q)
    return sums, np.bincount(assign[live], minlength=Kc).astype(np.int64)


def centroid_formula(sums, counts, before):
    c = np.maximum(counts, 1)[:, None].astype(np.float64)
    out = ((sums.astype(np.float64) / c) * 2.0 ** -24).astype(np.float32)
    return np.where(counts[:, None] > 0, out, before)


@pytest.mark.parametrize("operands", ["f16x3", "bf16x3"])
@pytest.mark.parametrize("D", [17, 40, 512])
@pytest.mark.parametrize("Kc", [1, 3, 130])
@pytest.mark.parametrize("n", [300, 301])
def test_assign_against_float64(cuda, n, Kc, D, operands):
    rng = np.random.default_rng(1000 * n + 10 * Kc + D)
    f = rng.standard_normal((n, D)).astype(np.float32)
    mu = rng.standard_normal((Kc, D)).astype(np.float32)
    assign, dist, sums, counts, bad = run_assign(cuda, f, mu, operands)
    assert bad[0] == 0 and assign.min() >= 0 and assign.max() < Kc
    d2 = d2_all(f, mu)
    rows = np.arange(n)
    eps = E_OP[operands] + (D + 2) * 2.0 ** -24
    bound = 2 * eps * ((f.astype(np.float64) ** 2).sum(axis=1)
                       + (mu.astype(np.float64) ** 2).sum(axis=1).max())
    excess = d2[rows, assign] - d2.min(axis=1)
    two = np.sort(np.concatenate([d2, np.full((n, 1), np.inf)], axis=1), axis=1)[:, :2]
    clear = two[:, 1] - two[:, 0] > bound
    print(f"excess / bound <= {(excess / bound).max():.3g}, clear {100 * clear.mean():.1f} %")
    assert np.all(excess <= bound) and clear.mean() >= 0.95
    assert np.array_equal(assign[clear], d2.argmin(axis=1)[clear])
    want = np.sqrt(d2[rows, assign])
    assert np.all(np.abs(dist - want) <= value_bound(D) * want)
    ref_sums, ref_counts = grouped(f, assign, Kc)
    assert np.array_equal(sums, ref_sums) and np.array_equal(counts, ref_counts)
    perm = rng.permutation(n)
    for got, order in ((run_assign(cuda, f, mu, operands, split=77), np.arange(n)),
                       (run_assign(cuda, f[perm], mu, operands), perm)):
        assert np.array_equal(got[0], assign[order]) and np.array_equal(got[2], sums)
        assert np.array_equal(got[1].view(np.uint32), dist[order].view(np.uint32))
        assert np.array_equal(got[3], counts)


def test_ties_and_duplicates(cuda):
    """Identical centroids in the other lane half (6) and in the next 128-centroid step (130): the
    smallest id wins; a row that equals a centroid scores exactly 0."""
    rng = np.random.default_rng(3)
    mu = rng.standard_normal((131, 40)).astype(np.float32)
    mu[6] = mu[130] = mu[2]
    near = rng.integers(0, 131, 200)
    near[3:10], near[10:20] = 6, 130
    f = (mu[near] + 0.01 * rng.standard_normal((200, 40))).astype(np.float32)
    f[:3] = mu[[2, 77, 130]]
    assign, dist, _, counts, _ = run_assign(cuda, f, mu)
    assert assign[:3].tolist() == [2, 77, 2] and dist[:3].tolist() == [0.0, 0.0, 0.0]
    assert np.all(assign[3:20] == 2) and counts[6] == 0 and counts[130] == 0
    assert np.array_equal(d2_all(f, mu).argmin(axis=1), assign)  # (argmin: the first minimum)


def test_bad_rows(cuda):
    rng = np.random.default_rng(4)
    f = rng.standard_normal((300, 40)).astype(np.float32)
    mu = rng.standard_normal((3, 40)).astype(np.float32)
    f[3, 39], f[130, 0], f[299, 17] = np.nan, np.inf, -2.0 ** 15
    assign, dist, sums, counts, bad = run_assign(cuda, f, mu)
    where = np.array([3, 130, 299])
    assert bad[0] == 3 and np.all(assign[where] == -1) and np.all(np.isnan(dist[where]))
    assert np.array_equal(np.flatnonzero(assign < 0), where) and counts.sum() == 297
    assert all(np.array_equal(x, y) for x, y in zip((sums, counts), grouped(f, assign, 3)))
    with pytest.raises(ValueError, match="3 feature row"):  # (the stand-alone function names them)
        forward_scores.kmeans(torch.from_numpy(f).to(cuda), 3, 1)


def test_centroids_formula_and_empty_cluster(cuda):
    rng = np.random.default_rng(5)
    sums = rng.integers(-2 ** 62, 2 ** 62, (5, 40), dtype=np.int64)
    counts = np.array([7, 0, 1, 2 ** 24 - 1, 300], np.int64)
    before = rng.standard_normal((5, 40)).astype(np.float32)
    got = _capi.kmeans_centroids(torch.from_numpy(sums).to(cuda), torch.from_numpy(counts).to(cuda),
                                 torch.from_numpy(before).to(cuda)).cpu().numpy()
    want = centroid_formula(sums, counts, before)
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))


def test_whole_lloyd_run_on_planted_blobs(cuda):
    """Four blobs 10 apart, noise 0.1, 301 rows in blob order: a seed row in every blob."""
    rng = np.random.default_rng(6)
    n, D, k, iters = 301, 40, 4, 5
    blob = np.arange(n) * k // n
    f = ((10 / np.sqrt(2)) * np.eye(k, D)[blob] + 0.1 * rng.standard_normal((n, D))).astype(
        np.float32)
    mu = f[forward_scores.kmeans_seed_rows(n, k)].astype(np.float64)
    for _ in range(iters):
        a = d2_all(f, mu).argmin(axis=1)
        mu = np.stack([f[a == j].astype(np.float64).mean(axis=0) for j in range(k)])
    runs = [[t.cpu().numpy() for t in forward_scores.kmeans(torch.from_numpy(f).to(cuda), k, iters)]
            for _ in range(2)]
    cent, assign, _ = runs[0]
    assert np.array_equal(assign, d2_all(f, mu).argmin(axis=1)) and np.array_equal(assign, blob)
    want = centroid_formula(*grouped(f, a, k), np.zeros((k, D), np.float32))
    assert np.array_equal(cent.view(np.uint32), want.view(np.uint32))
    for x, y in zip(*runs):
        assert np.array_equal(x.view(np.uint8), y.view(np.uint8))
