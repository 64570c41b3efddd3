"""The kmeans score through ScoringEngine (chunk sizes, lanes, two shards, beside el2n) and
sparse_loader: ResNet-18, K = 2 checkpoints, N = 300 (tests/test_gpu_proto_engine.py's shape)."""
import threading

import pytest
import torch

from data_diet_distributed_amd import checkpoints, forward_scores, synthetic
from data_diet_distributed_amd.get_scores_and_prune import sparse_loader
from data_diet_distributed_amd.loader import ArrayImageDataset, MyDataset
from data_diet_distributed_amd.scoring import ScoreConfig, ScoringEngine, shard_bounds

pytestmark = pytest.mark.gpu

N, C, KM, ITERS = 300, 10, 7, 4


@pytest.fixture(scope="module")
def case(cuda):
    images, labels = synthetic.make_images(N, C, seed=57)
    sds = [synthetic.make_checkpoint("resnet18", C, seed=s)["net"] for s in (11, 12)]
    return {"images": images, "labels": labels, "sds": sds,
            "models": checkpoints.build_models(sds, device=cuda),
            "img": torch.from_numpy(images).to(cuda), "lab": torch.from_numpy(labels).to(cuda)}


def shard(case, cuda, methods=("kmeans",), lo=0, hi=N, **kw):
    cfg = ScoreConfig(methods=methods, select_by=methods[0], kmeans_k=KM, kmeans_iters=ITERS,
                      **{"el2n_chunk": 128, **kw})  # (three launch chunks per checkpoint)
    return ScoringEngine(case["models"], cfg, cuda).score_shard(case["img"], case["lab"], lo, hi)


@pytest.fixture(scope="module")
def one(case, cuda):
    rows, inner = [], forward_scores.KMeansScore.end_checkpoint
    with pytest.MonkeyPatch.context() as mp:
        mp.setattr(forward_scores.KMeansScore, "end_checkpoint",
                   lambda self, f: (rows.append(f.clone()), inner(self, f))[1])
        return shard(case, cuda)["kmeans"], rows


def test_engine_equals_the_stand_alone_function(cuda, one):
    got, rows = one
    assert len(rows) == 2 and rows[0].shape == (N, 512)
    dists = [forward_scores.kmeans(f, KM, ITERS)[2] for f in rows]
    assert torch.equal(got, forward_scores.ensemble_mean(dists[0] + dists[1], 2))
    assert bool(torch.isfinite(got).all())


@pytest.mark.parametrize("kw", [{"el2n_chunk": 1024}, {"lanes": 3}], ids=["chunk", "lanes"])
def test_bitwise_across_launch_plans_and_beside_el2n(cuda, case, one, kw):
    both = shard(case, cuda, ("el2n", "kmeans"), **kw)
    assert torch.equal(both["kmeans"], one[0])
    assert torch.equal(both["el2n"], shard(case, cuda, ("el2n",))["el2n"])


def test_bitwise_across_two_shards(cuda, case, one, monkeypatch):
    """Two ranks as two threads that take turns (one lock) and meet in a stand-in all-reduce."""
    bounds = [shard_bounds(N, 128, 2, r) for r in range(2)]
    me, lock, gate = threading.local(), threading.Lock(), threading.Barrier(2, timeout=30)
    parts, out = [None, None], [None, None]

    def meet():
        lock.release()
        try:
            gate.wait()
        finally:
            lock.acquire()

    def all_reduce(t, group=None):
        parts[me.r] = t
        meet()
        total = parts[0] + parts[1]
        meet()
        t.copy_(total)

    def rank(r):
        me.r = r
        with lock:
            try:
                out[r] = shard(case, cuda, ("el2n", "kmeans"), *bounds[r])
            except BaseException:
                gate.abort()
                raise

    monkeypatch.setattr(forward_scores, "shard_lengths",
                        lambda n, group=None: ([b - a for a, b in bounds], me.r))
    monkeypatch.setattr(forward_scores, "_all_reduce_sum", all_reduce)
    threads = [threading.Thread(target=rank, args=(r,)) for r in range(2)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert torch.equal(torch.cat([out[0]["kmeans"], out[1]["kmeans"]]), one[0])


def test_sparse_loader_ranks_by_kmeans(cuda, case):
    from data_diet_distributed_amd.resnet import ResNet18
    net = ResNet18().to(cuda)
    net.load_state_dict(case["sds"][0])
    ds = MyDataset(ArrayImageDataset(case["images"], case["labels"]))
    loader = torch.utils.data.DataLoader(ds, batch_size=128, shuffle=False)
    _, samples, idx = sparse_loader(loader, N, net, cuda, 0.5, 128, 0, score="kmeans",
                                    kmeans_k=KM, kmeans_iters=ITERS, return_indices=True)
    assert samples == 150 and len(set(idx)) == 150 and set(idx) <= set(range(N))
