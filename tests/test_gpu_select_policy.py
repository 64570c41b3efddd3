"""Selection policies through the product layers: ScoringEngine.run, shards, sparse_loader and
the config entry point (ResNet-18, one synthetic checkpoint, N = 640, 10 classes, EL2N).
Keep-sets are compared bit-exactly with the NumPy restatement (tests/test_select_policy.py)
applied to the scores the run itself returned.
"""
import json
import os

import numpy as np
import pytest
import torch

from data_diet_distributed_amd import _capi, checkpoints, score, subset_index, synthetic
from data_diet_distributed_amd.get_scores_and_prune import (el2n_scores_from_loader,
                                                            sparse_loader)
from data_diet_distributed_amd.loader import ArrayImageDataset, MyDataset
from data_diet_distributed_amd.scoring import (ScoreConfig, ScoringEngine, apportion,
                                               select_with_policy, shard_bounds)
from test_select_policy import ref_select

pytestmark = pytest.mark.gpu

N, C, DATA_SEED, CKPT_SEED = 640, 10, 83, 29  # tests/helpers/policy_child.py uses the same


@pytest.fixture(scope="module")
def case(cuda):
    images, labels = synthetic.make_images(N, C, seed=DATA_SEED)
    sd = synthetic.make_checkpoint("resnet18", C, seed=CKPT_SEED)["net"]
    models = checkpoints.build_models([sd], device=cuda)
    img, lab = torch.from_numpy(images).to(cuda), torch.from_numpy(labels).to(cuda)
    return {"images": images, "labels": labels, "sd": sd, "models": models, "img": img,
            "lab": lab, "counts": np.bincount(labels, minlength=C).tolist()}


def test_engine_balanced_keeps_the_apportioned_quotas(cuda, case):
    eng = ScoringEngine(case["models"], ScoreConfig(select_policy="balanced"), cuda)
    full, kept, k = eng.run(case["img"], case["lab"], 0.5)
    kept = kept.cpu().numpy()
    assert k == 320 and len(kept) == k
    quota = apportion(k, case["counts"], "balanced")
    assert np.bincount(case["labels"][kept], minlength=C).tolist() == quota
    sel = eng.last_selection
    assert sel == {"policy": "balanced", "skip": 0, "class_counts": case["counts"],
                   "class_skip": [0] * C, "class_quota": quota}
    scores = full["el2n"].cpu().numpy()
    assert np.array_equal(kept, ref_select(scores, case["labels"], C, k, "balanced"))
    assert eng.last_refine is None


@pytest.mark.parametrize("policy,skip", [("stratified", 0), ("stratified", 50), ("balanced", 64),
                                         ("global", 40)])
def test_engine_policies_and_skips(cuda, case, policy, skip):
    eng = ScoringEngine(case["models"], ScoreConfig(select_policy=policy, select_skip=skip), cuda)
    full, kept, k = eng.run(case["img"], case["lab"], 0.7)
    scores = full["el2n"].cpu().numpy()
    want = ref_select(scores, case["labels"], C, k, policy, skip)
    assert len(want) == k and np.array_equal(kept.cpu().numpy(), want)
    assert eng.last_selection["policy"] == policy and eng.last_selection["skip"] == skip
    if policy == "global":
        top = _capi.select_topk(full["el2n"], skip + k)[0].cpu().numpy()
        assert np.array_equal(want, top[skip:])


def test_engine_default_selection_is_select_topk(cuda, case):
    eng = ScoringEngine(case["models"], ScoreConfig(), cuda)
    full, kept, k = eng.run(case["img"], case["lab"], 0.5)
    assert torch.equal(kept, _capi.select_topk(full["el2n"], k)[0])
    assert eng.last_selection["policy"] == "global" and eng.last_selection["skip"] == 0
    assert eng.last_selection["class_quota"] is None
    # ... and the class policies rank the very same scores
    eng_b = ScoringEngine(case["models"], ScoreConfig(select_policy="balanced"), cuda)
    assert torch.equal(eng_b.run(case["img"], case["lab"], 0.5)[0]["el2n"], full["el2n"])


def test_engine_skip_past_the_end_is_rejected(cuda, case):
    eng = ScoringEngine(case["models"], ScoreConfig(select_skip=400), cuda)
    with pytest.raises(ValueError, match="skip"):
        eng.run(case["img"], case["lab"], 0.5)  # 400 + 320 > 640


def test_engine_bad_label_raises_label_error(cuda, case):
    lab = case["lab"].clone()
    lab[77] = C
    eng = ScoringEngine(case["models"], ScoreConfig(select_policy="stratified"), cuda)
    with pytest.raises(_capi.LabelError):
        eng.run(case["img"], lab, 0.5)


@pytest.mark.parametrize("world", [2, 4])
def test_in_process_shards_select_like_world1(cuda, case, world):
    eng = ScoringEngine(case["models"], ScoreConfig(select_policy="balanced", select_skip=30),
                        cuda)
    full, kept, k = eng.run(case["img"], case["lab"], 0.6)
    parts, labs = [], []
    for r in range(world):
        lo, hi = shard_bounds(N, 128, world, r)
        parts.append(eng.score_shard(case["img"], case["lab"], lo, hi)["el2n"])
        labs.append(case["lab"][lo:hi])
    scores, labels = torch.cat(parts), torch.cat(labs)
    assert torch.equal(scores, full["el2n"])
    got, rec = select_with_policy(scores, labels, C, k, "balanced", 30)
    assert torch.equal(got, kept) and rec == eng.last_selection


def test_two_ranks_hold_their_shard_of_the_labels(cuda, case, tmp_path):
    """Two rank processes on cuda:0 in a gloo group, each holding ONLY its shard of the images
    and labels (run(n_total=N)): the labels are gathered for the class policy and every rank
    selects what the single-process run selects (tests/helpers/policy_child.py)."""
    from data_diet_distributed_amd import launch
    child = os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers",
                         "policy_child.py")
    out = str(tmp_path / "w2.npz")
    assert launch.launch_ranks(2, [child, out]) == 0
    w2 = np.load(out)
    eng = ScoringEngine(case["models"], ScoreConfig(select_policy="stratified", select_skip=25),
                        cuda)
    full, kept, k = eng.run(case["img"], case["lab"], 0.5)
    assert int(w2["world"]) == 2 and int(w2["k"]) == k
    assert np.array_equal(w2["el2n"], full["el2n"].cpu().numpy())
    assert np.array_equal(w2["kept"], kept.cpu().numpy())
    assert w2["class_quota"].tolist() == eng.last_selection["class_quota"]
    assert w2["class_skip"].tolist() == eng.last_selection["class_skip"]


def _loader_and_net(case, cuda):
    from data_diet_distributed_amd.resnet import ResNet18
    net = ResNet18().to(cuda)
    net.load_state_dict(case["sd"])  # train mode, as the reference scores
    ds = MyDataset(ArrayImageDataset(case["images"], case["labels"]))
    return torch.utils.data.DataLoader(ds, batch_size=128, shuffle=False), net


def test_sparse_loader_stratified_on_both_paths(cuda, case, tmp_path):
    k = _capi.keep_count(N, 0.5)
    quota = apportion(k, case["counts"], "stratified")
    for fast in (True, False):
        loader, net = _loader_and_net(case, cuda)
        path = str(tmp_path / f"keep_{int(fast)}")
        _, samples, idx = sparse_loader(loader, N, net, cuda, 0.5, 128, 0, fast=fast,
                                        policy="stratified", return_indices=True,
                                        subset_index_path=path)
        assert sparse_loader.last_path == ("fast" if fast else "general")
        assert samples == k and len(idx) == k and len(set(idx)) == k
        assert np.bincount(case["labels"][idx], minlength=C).tolist() == quota
        assert sparse_loader.last_selection["class_quota"] == quota
        meta = subset_index.read_subset_index(path)[1]
        assert meta["select_policy"] == "stratified" and meta["select_skip"] == 0
        assert meta["class_quota"] == quota and meta["class_skip"] == [0] * C
    # the general path's keep-set is the restatement on the scores of its own forward
    loader, net = _loader_and_net(case, cuda)
    s, v = el2n_scores_from_loader(loader, net, cuda)
    assert v.cpu().tolist() == list(range(N))
    assert idx == ref_select(s.cpu().numpy(), case["labels"], C, k, "stratified").tolist()


def test_sparse_loader_skip_and_defaults(cuda, case, tmp_path):
    loader, net = _loader_and_net(case, cuda)
    _, _, base = sparse_loader(loader, N, net, cuda, 0.5, 128, 0, return_indices=True,
                               subset_index_path=str(tmp_path / "d"))
    assert sparse_loader.last_selection is None
    meta = subset_index.read_subset_index(str(tmp_path / "d"))[1]
    assert not {"select_policy", "select_skip", "class_quota", "class_skip"} & set(meta)
    loader, net = _loader_and_net(case, cuda)
    _, _, win = sparse_loader(loader, N, net, cuda, 0.75, 128, 0, return_indices=True, skip=100)
    assert win == base[100:260]  # global ranks [100, 260) of the same scores
    with pytest.raises(ValueError, match="refine"):
        sparse_loader(loader, N, net, cuda, 0.5, 128, 0, refine=True, policy="balanced")
    with pytest.raises(ValueError):
        sparse_loader(loader, N, net, cuda, 0.5, 128, 0, policy="per_class")


def test_config_entry_writes_the_selection_metadata(cuda, case, tmp_path):
    ck = tmp_path / "checkpoint"
    os.makedirs(ck)
    torch.save({"net": case["sd"], "acc": 0.0, "epoch": 19}, ck / "ckpt_19.pth")
    base = (f"dataset: synthetic-cifar10\nsynthetic_n: {N}\nsynthetic_seed: {DATA_SEED}\n"
            f"batch_size: 128\nsparsity: 0.5\ncheckpoint_path: {ck}\n")
    new_keys = {"select_policy", "select_skip", "class_quota", "class_skip"}
    (tmp_path / "b.yaml").write_text(base + "select_policy: balanced\n")
    out_b = str(tmp_path / "idx" / "balanced")
    assert score.main(["--config", str(tmp_path / "b.yaml"), "--out", out_b]) == 0
    idx, meta = subset_index.read_subset_index(out_b)
    quota = apportion(320, case["counts"], "balanced")
    assert new_keys <= set(meta)
    assert meta["select_policy"] == "balanced" and meta["select_skip"] == 0
    assert meta["class_quota"] == quota and meta["class_skip"] == [0] * C and meta["k"] == 320
    assert np.bincount(case["labels"][idx], minlength=C).tolist() == meta["class_quota"]
    # the command-line override of a default config, and the default run's metadata
    (tmp_path / "d.yaml").write_text(base)
    out_s = str(tmp_path / "idx" / "cli")
    assert score.main(["--config", str(tmp_path / "d.yaml"), "--out", out_s, "--policy",
                       "balanced"]) == 0
    assert np.array_equal(subset_index.read_subset_index(out_s)[0], idx)
    out_d = str(tmp_path / "idx" / "default")
    assert score.main(["--config", str(tmp_path / "d.yaml"), "--out", out_d]) == 0
    with open(out_d + ".json") as f:
        meta_d = json.load(f)
    assert not new_keys & set(meta_d)
