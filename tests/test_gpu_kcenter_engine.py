"""The kcenter fill through the product layers: ScoringEngine.run (the feature rows of
kcenter_ckpt kept from the EL2N forward, chunk sizes, lanes, n_total mode, two ranks),
sparse_loader and the config entry.  The case of tests/test_gpu_knn_engine.py: ResNet-18, K = 3
synthetic checkpoints, N = 300 = two full batches of 128 + a ragged 44, 10 classes, el2n_chunk =
128; the rows the picks are checked on are those the run itself produced, recorded by wrapping
the forward (that file's Recorder).

The greedy check and the bound g = (D + 2) 2^-24 are those of tests/test_gpu_kcenter.py; the
radius is the square root of a squared distance within g of float64, hence within g too.
"""
import os

import numpy as np
import pytest
import torch

from data_diet_distributed_amd import _capi, checkpoints, methods, scoring, score
from data_diet_distributed_amd import subset_index, synthetic
from data_diet_distributed_amd.get_scores_and_prune import sparse_loader
from data_diet_distributed_amd.loader import ArrayImageDataset, MyDataset
from data_diet_distributed_amd.scoring import ScoreConfig, ScoringEngine, apportion, shard_bounds
from test_gpu_knn_engine import Recorder
from test_kcenter_select import check_greedy

pytestmark = pytest.mark.gpu

N, C, K, D = 300, 10, 3, 512
G_BOUND = (D + 2) * 2.0 ** -24
FRAC = 0.1


@pytest.fixture(scope="module")
def case(cuda):
    images, labels = synthetic.make_images(N, C, seed=57)
    sds = [synthetic.make_checkpoint("resnet18", C, seed=s)["net"] for s in (11, 12, 13)]
    return {"images": images, "labels": labels, "sds": sds,
            "models": checkpoints.build_models(sds, device=cuda),
            "img": torch.from_numpy(images).to(cuda), "lab": torch.from_numpy(labels).to(cuda)}


def engine(case, cuda, **kw):
    kw.setdefault("el2n_chunk", 128)  # three launch chunks per checkpoint
    kw.setdefault("methods", ("el2n",))
    kw.setdefault("select_fill", "kcenter")
    kw.setdefault("kcenter_seed_frac", FRAC)
    return ScoringEngine(case["models"], ScoreConfig(**kw), cuda)


def check_selection(kept, k, keys, rows, labels, policy, rec, dev, frac=FRAC):
    """The keep-set `kept` of a kcenter selection of k of the examples with scores `keys`
    (device) and float32 rows `rows` [n, D] (NumPy) against the semantics: k unique indices,
    the quotas, the seeds = the score cut's top m_g, every pick greedy in float64 within the
    bound, and the recorded radius."""
    n = len(rows)
    kept = kept.cpu().numpy()
    assert len(kept) == k and len(set(kept.tolist())) == k
    if policy == "global":
        groups, sizes, quotas = np.zeros(n, np.int64), [n], [k]
    else:
        groups = np.asarray(labels)
        sizes = np.bincount(groups, minlength=C).tolist()
        quotas = apportion(k, sizes, policy)
        assert rec["class_quota"] == quotas
        assert np.bincount(groups[kept], minlength=C).tolist() == quotas
    G = len(sizes)
    m = methods.seed_counts(quotas, frac)
    assert rec["fill"] == "kcenter" and rec["class_seeds"] == m and rec["policy"] == policy
    if policy == "global":
        want = _capi.select_topk(keys, m[0])[0]
    else:
        lab_d = torch.from_numpy(groups).to(dev)
        want = _capi.select_topk_by_class(keys, lab_d, C, [0] * C, m)[0]
    seeds = kept[:sum(m)]
    assert np.array_equal(seeds, want.cpu().numpy())  # the score cut, in its order
    picks = [q - a for q, a in zip(quotas, m)]
    steps = max(picks)
    picked = np.full((steps, G), -1, dtype=np.int64)
    rest = iter(kept[sum(m):].tolist())
    for t in range(steps):  # the kept order of the picks: by (step, group)
        for g in range(G):
            if t < picks[g]:
                picked[t, g] = next(rest)
    assert next(rest, None) is None
    _, final = check_greedy(rows, np.arange(n), groups, seeds, picks, picked,
                            slack=1.0 - (1.0 - G_BOUND) / (1.0 + G_BOUND))
    for g in range(G):
        mine = final[groups == g]
        r64 = float(np.sqrt(mine.max())) if len(mine) and mine.max() > 0 else 0.0
        if np.isinf(r64):  # a group that keeps none of its rows
            assert np.isposinf(rec["radius"][g])
            continue
        assert abs(rec["radius"][g] - r64) <= G_BOUND * r64, (g, rec["radius"][g], r64)
    return picked


@pytest.mark.parametrize("ckpt", [-1, 0], ids=["last", "ckpt0"])
@pytest.mark.parametrize("policy", ["global", "balanced"])
def test_run_with_the_kcenter_fill(cuda, case, monkeypatch, policy, ckpt):
    rec = Recorder(monkeypatch)
    eng = engine(case, cuda, select_policy=policy, kcenter_ckpt=ckpt)
    full, kept, k = eng.run(case["img"], case["lab"], 0.5)
    assert k == 150 and len(rec.calls) == K * 3  # still one forward per checkpoint and chunk
    assert eng.last_refine is None
    feats = rec.features(case["models"])
    assert feats.shape == (K, N, D) and feats.dtype == np.float32
    check_selection(kept, k, full["el2n"], feats[ckpt], case["labels"], policy,
                    eng.last_selection, cuda)
    if ckpt == -1:
        # the rows of another checkpoint give another keep-set (the option is not ignored)
        other = engine(case, cuda, select_policy=policy, kcenter_ckpt=0)
        assert not torch.equal(other.run(case["img"], case["lab"], 0.5)[1], kept)


def test_keep_set_is_bitwise_invariant(cuda, case):
    """The chunk size, lanes, the n_total mode and other requested scores change no bit of the
    keep-set or of the radii."""
    img, lab = case["img"], case["lab"]
    for policy in ("global", "balanced"):
        eng = engine(case, cuda, select_policy=policy)
        _, kept, k = eng.run(img, lab, 0.5)
        radius = eng.last_selection["radius"]
        for kw in ({"el2n_chunk": 256}, {"el2n_chunk": 1024}, {"lanes": 2},
                   {"methods": ("el2n", "proto", "knn"), "select_by": "el2n"}):
            other = engine(case, cuda, select_policy=policy, **kw)
            assert torch.equal(other.run(img, lab, 0.5)[1], kept), (policy, kw)
            assert other.last_selection["radius"] == radius, (policy, kw)
        shard = engine(case, cuda, select_policy=policy)
        assert torch.equal(shard.run(img, lab, 0.5, n_total=N)[1], kept), policy


def test_score_fill_is_todays_selection(cuda, case):
    img, lab = case["img"], case["lab"]
    for kw in ({}, {"select_policy": "stratified"}, {"select_policy": "balanced",
                                                       "select_skip": 7}):
        plain = ScoringEngine(case["models"], ScoreConfig(methods=("el2n", "proto"),
                                                          el2n_chunk=128, **kw), cuda)
        named = ScoringEngine(case["models"], ScoreConfig(
            methods=("el2n", "proto"), el2n_chunk=128, select_fill="score",
            kcenter_seed_frac=0.5, kcenter_ckpt=0, **kw), cuda)
        a, b = plain.run(img, lab, 0.5), named.run(img, lab, 0.5)
        assert a[2] == b[2] and torch.equal(a[1], b[1]), kw
        for m in a[0]:
            assert torch.equal(a[0][m], b[0][m]), (kw, m)
        assert named.last_selection == plain.last_selection  # the record is today's too
        assert not {"fill", "class_seeds", "radius"} & set(named.last_selection)
        assert named._kcenter_rows is None  # no rows are kept for the score fill


def test_non_finite_rows_raise_with_their_count(cuda, case):
    keys = torch.rand(N, device=cuda)
    rows = torch.rand((N, 64), device=cuda)
    rows[5, 3] = float("nan")
    rows[9, 0] = float("inf")
    with pytest.raises(ValueError, match="2 feature row"):
        scoring.select_with_policy(keys, None, None, 50, fill="kcenter", rows=rows)
    with pytest.raises(ValueError, match="rows"):
        scoring.select_with_policy(keys, None, None, 50, fill="kcenter")
    with pytest.raises(ValueError, match="skip"):
        scoring.select_with_policy(keys, None, None, 50, skip=1, fill="kcenter", rows=rows)
    keys[17] = float("nan")
    with pytest.raises(ValueError, match="NaN score"):
        scoring.select_with_policy(keys, None, None, 50, fill="kcenter",
                                   rows=torch.rand((N, 64), device=cuda))


@pytest.mark.parametrize("policy", ["balanced"])
def test_two_ranks_equal_world1_bitwise(cuda, tmp_path, policy):
    """Two rank processes on cuda:0 over gloo, each holding only its shard: every rank runs the
    identical selection on the gathered rows, so the keep-set equals the single-process run's
    bit for bit."""
    from data_diet_distributed_amd import launch
    from helpers import kcenter_child
    n = 5 * 128 + 40  # shards [0, 384), [384, 680)
    out = str(tmp_path / "w2.npz")
    assert launch.launch_ranks(2, [os.path.abspath(kcenter_child.__file__), out, str(n),
                                   policy]) == 0
    w2 = np.load(out)
    assert int(w2["world"]) == 2 and w2["shard"].tolist() == list(shard_bounds(n, 128, 2, 0))
    images, labels = synthetic.make_images(n, 10, seed=kcenter_child.DATA_SEED)
    sds = [synthetic.make_checkpoint("resnet18", 10, seed=s)["net"]
           for s in kcenter_child.CKPT_SEEDS]
    eng = ScoringEngine(checkpoints.build_models(sds, device=cuda),
                        kcenter_child.config(policy), cuda)
    full, kept, k = eng.run(torch.from_numpy(images).to(cuda), torch.from_numpy(labels).to(cuda),
                            kcenter_child.SPARSITY)
    assert np.array_equal(w2["el2n"], full["el2n"].cpu().numpy())
    assert int(w2["k"]) == k and np.array_equal(w2["kept"], kept.cpu().numpy())
    assert w2["radius"].tolist() == eng.last_selection["radius"]
    assert w2["class_seeds"].tolist() == eng.last_selection["class_seeds"]


def test_outer_layers(cuda, case, tmp_path, monkeypatch):
    from data_diet_distributed_amd.resnet import ResNet18
    net = ResNet18().to(cuda)
    net.load_state_dict(case["sds"][0])
    ds = MyDataset(ArrayImageDataset(case["images"], case["labels"]))
    loader = torch.utils.data.DataLoader(ds, batch_size=128, shuffle=False)
    seen = []
    inner = scoring.select_with_policy

    def recording(keys, labels, num_classes, k, policy="global", skip=0, check_nan=True, **kw):
        seen.append((keys.clone(), None if labels is None else labels.cpu().numpy().copy(),
                     kw["rows"].cpu().numpy().copy(), kw["fill"], kw["seed_frac"]))
        return inner(keys, labels, num_classes, k, policy, skip, check_nan, **kw)

    monkeypatch.setattr(scoring, "select_with_policy", recording)
    for fast in (True, False):
        for policy in ("global", "stratified"):
            seen.clear()
            _, samples, idx = sparse_loader(loader, N, net, cuda, 0.5, 128, 0, fast=fast,
                                            return_indices=True, policy=policy, fill="kcenter",
                                            seed_frac=0.2)
            assert sparse_loader.last_path == ("fast" if fast else "general")
            assert samples == 150 and len(seen) == 1
            keys, labels, rows, fill, frac = seen[0]
            assert fill == "kcenter" and frac == 0.2 and rows.shape == (N, D)
            # the visit order is the dataset's: the standalone selection on the visited rows
            check_selection(torch.tensor(idx), 150, keys, rows, case["labels"], policy,
                            sparse_loader.last_selection, cuda, frac=0.2)
            assert sparse_loader.last_refine is None
    monkeypatch.setattr(scoring, "select_with_policy", inner)
    with pytest.raises(ValueError, match="refine"):
        sparse_loader(loader, N, net, cuda, 0.5, 128, 0, fill="kcenter", refine=True)
    with pytest.raises(ValueError, match="skip"):
        sparse_loader(loader, N, net, cuda, 0.5, 128, 0, fill="kcenter", skip=2)
    # the config entry: the keys and --fill reach the engine and the metadata
    ck = tmp_path / "checkpoint"
    os.makedirs(ck)
    torch.save({"net": case["sds"][0], "acc": 0.0, "epoch": 19}, ck / "ckpt_19.pth")
    (tmp_path / "p.yaml").write_text(
        f"dataset: synthetic-cifar10\nsynthetic_n: {N}\nsynthetic_seed: 57\nbatch_size: 128\n"
        f"sparsity: 0.5\ncheckpoint_path: {ck}\nselect_policy: balanced\n"
        f"kcenter_seed_frac: 0.2\n")
    out = str(tmp_path / "idx" / "kc")
    assert score.main(["--config", str(tmp_path / "p.yaml"), "--out", out, "--fill",
                       "kcenter"]) == 0
    idx, meta = subset_index.read_subset_index(out)
    assert meta["select_fill"] == "kcenter" and meta["kcenter_seed_frac"] == 0.2
    assert meta["kcenter_ckpt"] == 0 and meta["k"] == 150 and len(set(idx.tolist())) == 150
    assert len(meta["radius"]) == C and len(meta["class_seeds"]) == C
    out2 = str(tmp_path / "idx" / "plain")
    assert score.main(["--config", str(tmp_path / "p.yaml"), "--out", out2]) == 0
    meta2 = subset_index.read_subset_index(out2)[1]
    assert not {"select_fill", "kcenter_seed_frac", "kcenter_ckpt", "radius",
                "class_seeds"} & set(meta2)
