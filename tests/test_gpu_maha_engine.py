"""The maha score through ScoringEngine (chunk sizes, lanes, beside el2n) and sparse_loader:
ResNet-18, K = 2, N = 300, D = 512 > N - C: the default shrinkage carries the factorisation."""
import numpy as np
import pytest
import torch

from data_diet_distributed_amd import _capi, checkpoints, forward_scores, synthetic
from data_diet_distributed_amd.get_scores_and_prune import sparse_loader
from data_diet_distributed_amd.loader import ArrayImageDataset, MyDataset
from data_diet_distributed_amd.scoring import ScoreConfig, ScoringEngine
from test_maha_scores import dist_bound, ref_maha, whitening_bound

pytestmark = pytest.mark.gpu

N, C = 300, 10


@pytest.fixture(scope="module")
def case(cuda):
    images, labels = synthetic.make_images(N, C, seed=57)
    sds = [synthetic.make_checkpoint("resnet18", C, seed=s)["net"] for s in (11, 12)]
    return {"images": images, "labels": labels, "sds": sds,
            "models": checkpoints.build_models(sds, device=cuda),
            "img": torch.from_numpy(images).to(cuda), "lab": torch.from_numpy(labels).to(cuda)}


def shard(case, cuda, methods=("el2n", "maha"), **kw):
    cfg = ScoreConfig(methods=methods, select_by="maha", **{"el2n_chunk": 128, **kw})
    return ScoringEngine(case["models"], cfg, cuda).score_shard(case["img"], case["lab"], 0, N)


@pytest.fixture(scope="module")
def one(case, cuda):
    rows, inner = [], forward_scores.MahaScore.end_checkpoint
    with pytest.MonkeyPatch.context() as mp:
        mp.setattr(forward_scores.MahaScore, "end_checkpoint",
                   lambda self, f, allf: (rows.append(f.clone()), inner(self, f, allf))[1])
        return shard(case, cuda), rows


def test_engine_agrees_with_the_restatement_on_its_own_rows(cuda, case, one):
    got, rows = one
    assert len(rows) == 2 and rows[0].shape == (N, 512)
    seg, want, bound = _capi.maha_segment_rows(N, 512), np.zeros(N), np.zeros(N)
    for f in rows:
        ref = ref_maha(f.cpu().numpy(), case["labels"], C, 0.01)
        b2 = dist_bound(ref, "f16x3") + whitening_bound(ref, "f16x3", seg, 0.01)
        want += ref["maha"] / 2
        bound += b2 / (2 * ref["maha"]) / 2  # |d - d64| <= |d^2 - d64^2| / (d + d64) ~ b2 / 2 d64
    err = np.abs(got["maha"].cpu().numpy().astype(np.float64) - want)
    print(f"engine: largest error / bound {np.max(err / bound):.3f}, "
          f"median bound / score {np.median(bound / want):.2e}")
    assert np.all(err <= 1.01 * bound)  # (1.01: d + d64 for 2 d64, and the mean's two roundings)
    stand_alone = [forward_scores.maha(f, case["lab"], C) for f in rows]
    assert torch.equal(got["maha"], forward_scores.ensemble_mean(sum(stand_alone), 2))


@pytest.mark.parametrize("kw", [{"el2n_chunk": 1024}, {"lanes": 3}], ids=["chunk", "lanes"])
def test_bitwise_across_launch_plans(cuda, case, one, kw):
    both = shard(case, cuda, **kw)
    assert torch.equal(both["maha"], one[0]["maha"]) and torch.equal(both["el2n"], one[0]["el2n"])


def test_beside_proto_the_class_means_are_shared(cuda, case, one):
    both = shard(case, cuda, ("proto", "maha"))
    assert torch.equal(both["maha"], one[0]["maha"]) and bool(torch.isfinite(both["proto"]).all())


def test_sparse_loader_ranks_by_maha(cuda, case):
    from data_diet_distributed_amd.resnet import ResNet18
    net = ResNet18().to(cuda)
    net.load_state_dict(case["sds"][0])
    ds = MyDataset(ArrayImageDataset(case["images"], case["labels"]))
    loader = torch.utils.data.DataLoader(ds, batch_size=128, shuffle=False)
    _, samples, idx = sparse_loader(loader, N, net, cuda, 0.5, 128, 0, score="maha",
                                    maha_shrink=0.05, return_indices=True)
    assert samples == 150 and len(set(idx)) == 150 and set(idx) <= set(range(N))
    with pytest.raises(ValueError, match="maha_shrink"):
        sparse_loader(loader, N, net, cuda, 0.5, 128, 0, score="maha", maha_shrink=2)
