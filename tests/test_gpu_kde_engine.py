"""The density scores through the product layers: ScoringEngine (chunk sizes and lanes change no
bit; the scores against the restatement of tests/test_kde_scores.py on the rows the run itself
gathered) and sparse_loader.  The case of tests/test_gpu_knn_engine.py: ResNet-18, K = 3 synthetic
checkpoints, N = 300 = two full batches of 128 + a ragged 44, 10 classes.

The bound on the engine's vectors: per checkpoint that of tests/test_kde_scores.py, the reference
taking inv as the kernel does (1 / (tau s) from a float64 s, rounded to fp32 once); the mean over K
adds (K + 2) 2^-23 of the value.
"""
import numpy as np
import pytest
import torch

from data_diet_distributed_amd import _capi, checkpoints, forward_scores, scoring, synthetic
from data_diet_distributed_amd.get_scores_and_prune import sparse_loader
from data_diet_distributed_amd.loader import ArrayImageDataset, MyDataset
from data_diet_distributed_amd.scoring import ScoreConfig, ScoringEngine
from test_kde_scores import kde_bound, ref_kde, ref_scale

pytestmark = pytest.mark.gpu

N, C, K = 300, 10, 3
KDE = ("kde", "kde_post")


@pytest.fixture(scope="module")
def case(cuda):
    images, labels = synthetic.make_images(N, C, seed=57)
    sds = [synthetic.make_checkpoint("resnet18", C, seed=s)["net"] for s in (11, 12, 13)]
    return {"images": images, "labels": labels, "sds": sds,
            "models": checkpoints.build_models(sds, device=cuda),
            "img": torch.from_numpy(images).to(cuda), "lab": torch.from_numpy(labels).to(cuda)}


def test_engine_scores_are_invariant_and_within_the_bound(cuda, case, monkeypatch):
    saved, inner = [], scoring.gather_rows

    def recording(t, lengths, group=None):
        if t.dim() == 2:
            saved.append(t.cpu().numpy().copy())
        return inner(t, lengths, group)

    def run(**kw):
        cfg = ScoreConfig(methods=("el2n",) + KDE, select_by="kde", **kw)
        return ScoringEngine(case["models"], cfg, cuda).score_shard(case["img"], case["lab"], 0, N)

    monkeypatch.setattr(forward_scores, "gather_rows", recording)
    one = run(el2n_chunk=128)
    monkeypatch.setattr(forward_scores, "gather_rows", inner)
    assert len(saved) == K and saved[0].shape == (N, 512)
    for kw in ({"el2n_chunk": 256}, {"el2n_chunk": 128, "lanes": 2}):
        got = run(**kw)
        for m in ("el2n",) + KDE:
            assert torch.equal(got[m], one[m]), (kw, m)
    want, bound = np.zeros((2, N)), np.zeros(N)
    for f in saved:
        inv = float(np.float32(1.0 / (0.25 * ref_scale(f))))
        nll, post, _ = ref_kde(f, case["labels"], None, inv=inv)
        want += np.stack([nll + np.log(N - 1), post]) / K
        bound += kde_bound(f, inv) / K
    for i, m in enumerate(KDE):
        err = np.abs(one[m].cpu().numpy() - want[i])
        b = (1 + i) * bound + (K + 2) * 2.0 ** -23 * np.abs(want[i])
        print(f"{m}: scores {want[i].min():.3g} .. {want[i].max():.3g}, worst error "
              f"{err.max():.3g}, error / bound <= {(err / b).max():.3g}")
        assert np.all(np.isfinite(want[i])) and np.all(err <= b), m
    wide = run(el2n_chunk=128, kde_bandwidth=1.0)["kde"]  # the bandwidth reaches the kernel
    assert not torch.equal(wide, one["kde"])


def test_sparse_loader_keeps_the_top_rows(cuda, case, monkeypatch):
    from data_diet_distributed_amd.resnet import ResNet18
    net = ResNet18().to(cuda)
    net.load_state_dict(case["sds"][0])
    ds = MyDataset(ArrayImageDataset(case["images"], case["labels"]))
    loader = torch.utils.data.DataLoader(ds, batch_size=128, shuffle=False)
    seen, inner = [], forward_scores.density

    def recording(*a, **kw):
        seen.append(inner(*a, **kw))
        return seen[-1]

    monkeypatch.setattr(forward_scores, "density", recording)
    for which, name in enumerate(KDE):
        _, samples, idx = sparse_loader(loader, N, net, cuda, 0.5, 128, 0, score=name,
                                        return_indices=True)
        assert samples == 150 and sparse_loader.last_path == "fast"
        # the visit order is the dataset's: the keep-set is the top half of that vector
        assert idx == _capi.select_topk(seen[-1][which], 150)[0].cpu().tolist()
