"""The prototype-distance score through the product layers: ScoringEngine (the feature tap of the
shared forward, the two-phase checkpoint, lanes, chunk sizes, the general path, ResNet-50,
selection, the fp16 fallback, two ranks), sparse_loader and the config entry.  ResNet-18, K = 3
synthetic checkpoints, N = 300 = two full batches of 128 + a ragged 44, 10 classes (the shape of
tests/test_gpu_logit_engine.py).  Scores are compared with the NumPy restatement
(tests/test_proto_scores.py) applied to the feature rows the run itself produced, recorded by
wrapping the forward.
"""
import os

import numpy as np
import pytest
import torch

from data_diet_distributed_amd import _capi, checkpoints, el2n_fast, score, subset_index, synthetic
from data_diet_distributed_amd.get_scores_and_prune import sparse_loader
from data_diet_distributed_amd.loader import ArrayImageDataset, MyDataset
from data_diet_distributed_amd.resnet import ResNet
from data_diet_distributed_amd.scoring import (FORWARD_FAMILY, LOGIT_FAMILY, ScoreConfig,
                                               ScoringEngine, shard_bounds)
from test_proto_scores import bound_ensemble, exact_class_means, ref_proto
from test_select_policy import ref_select

pytestmark = pytest.mark.gpu

N, C, K = 300, 10, 3


@pytest.fixture(scope="module")
def case(cuda):
    images, labels = synthetic.make_images(N, C, seed=57)
    sds = [synthetic.make_checkpoint("resnet18", C, seed=s)["net"] for s in (11, 12, 13)]
    return {"images": images, "labels": labels, "sds": sds,
            "models": checkpoints.build_models(sds, device=cuda),
            "img": torch.from_numpy(images).to(cuda), "lab": torch.from_numpy(labels).to(cuda)}


def engine(case, cuda, methods, models=None, **kw):
    kw.setdefault("el2n_chunk", 128)  # three launch chunks per checkpoint
    kw.setdefault("select_by", methods[0])
    return ScoringEngine(models or case["models"], ScoreConfig(methods=methods, **kw), cuda)


class Recorder:
    """Wraps el2n_fast.forward_features (forward_logits goes through it too): counts the calls
    and keeps each call's valid feature rows."""

    def __init__(self, monkeypatch):
        self.calls = []
        inner = el2n_fast.forward_features

        def wrapped(model, x, group_size, n_valid):
            logits, feat = inner(model, x, group_size, n_valid)
            self.calls.append((id(model), feat[:n_valid].cpu().numpy().copy()))
            return logits, feat

        monkeypatch.setattr(el2n_fast, "forward_features", wrapped)

    def features(self, models):
        """[K, rows, D]: each model's recorded chunks in call order."""
        return np.stack([np.concatenate([f for mid, f in self.calls if mid == id(m)])
                         for m in models])


def check_proto(got, feature_sets, labels, num_classes, what=""):
    """The engine's proto vector against the restatement on `feature_sets` [K, n, D]."""
    Kc, _, D = feature_sets.shape
    assert feature_sets.dtype == np.float32
    ref = ref_proto(feature_sets, labels, num_classes)
    mu_max = max(np.abs(exact_class_means(f, labels, num_classes)).max() for f in feature_sets)
    bound = bound_ensemble(D, ref, mu_max, Kc)
    err = np.abs(got.cpu().numpy().astype(np.float64) - ref)
    print(f"proto {what}: D={D} K={Kc} largest error / bound = {(err / bound).max():.3g}, "
          f"scores {ref.min():.3g} .. {ref.max():.3g}")
    assert np.all(err <= bound)
    assert ref.max() > 0  # (a class of one member sits on its prototype: distance 0)


def test_proto_against_recorded_features(cuda, case, monkeypatch):
    methods = LOGIT_FAMILY + ("proto", "grand")
    only = engine(case, cuda, ("el2n",)).run(case["img"], case["lab"], 0.5)[0]["el2n"]
    rec = Recorder(monkeypatch)
    full, kept, k = engine(case, cuda, methods).run(case["img"], case["lab"], 0.5)
    assert set(full) == set(methods) and all(v.numel() == N for v in full.values())
    assert len(rec.calls) == K * 3  # still one forward per checkpoint and chunk
    assert torch.equal(full["el2n"], only)
    assert all(bool(torch.isfinite(v).all()) for v in full.values())
    feats = rec.features(case["models"])
    assert feats.shape == (K, N, 512)
    check_proto(full["proto"], feats, case["labels"], C, "resnet18")


def test_forward_logits_is_the_first_output(cuda, case):
    m = case["models"][0]
    x = torch.randn(128, 3, 32, 32, device=cuda)
    logits, feat = el2n_fast.forward_features(m, x, 128, 100)
    assert feat.shape == (128, 512) and feat.dtype == torch.float32 and feat.is_contiguous()
    assert torch.equal(el2n_fast.forward_logits(m, x, 128, 100), logits)


def test_proto_is_bitwise_invariant(cuda, case):
    """Lanes, the chunk size and concurrent passes change no bit of any family member: the
    class sums are exact integers and every row's distance is reduced from that row alone."""
    img, lab = case["img"], case["lab"]
    one = engine(case, cuda, FORWARD_FAMILY).score_shard(img, lab, 0, N)
    for kw in ({"lanes": 3}, {"el2n_chunk": 1024}):
        got = engine(case, cuda, FORWARD_FAMILY, **kw).score_shard(img, lab, 0, N)
        for m in FORWARD_FAMILY:
            assert torch.equal(got[m], one[m]), (kw, m)
    methods = FORWARD_FAMILY + ("grand",)
    seq = engine(case, cuda, methods).score_shard(img, lab, 0, N)
    conc = engine(case, cuda, methods, concurrent_passes=True).score_shard(img, lab, 0, N)
    for m in methods:
        assert torch.equal(conc[m], seq[m]), m
        if m != "grand":
            assert torch.equal(seq[m], one[m]), m
    # a direct shard call without a group takes its prototypes over the shard only
    part = engine(case, cuda, ("proto",)).score_shard(img, lab, 0, 256)
    assert not torch.equal(part["proto"], one["proto"][:256])


@pytest.mark.parametrize("kw", [{"fast_el2n": False}, {"el2n_bn": "running"}],
                         ids=["fast_el2n_off", "running_bn"])
def test_general_path(cuda, case, monkeypatch, kw):
    """model.run per batch (no grouped forward): the features are the classifier's input rows
    on that path's tape, again from one forward per checkpoint and batch."""
    calls = []
    inner = ResNet.run

    def wrapped(self, x, *a, **k):
        out = inner(self, x, *a, **k)
        nv = k.get("n_valid")
        feat = k["tape"][-1][1]
        calls.append((id(self), feat[:nv if nv is not None else feat.shape[0]].float().cpu()
                      .numpy().copy()))
        return out

    monkeypatch.setattr(ResNet, "run", wrapped)
    full = engine(case, cuda, ("el2n", "proto"), **kw).score_shard(case["img"], case["lab"], 0, N)
    assert len(calls) == K * 3  # one forward per checkpoint and batch
    sets = np.stack([np.concatenate([f for mid, f in calls if mid == id(m)])
                     for m in case["models"]])
    assert sets.shape == (K, N, 512)
    check_proto(full["proto"], sets, case["labels"], C, str(kw))


def test_resnet50_wide_features_from_the_torch_pool(cuda, monkeypatch):
    """ResNet-50, 100 classes, K = 1, N = 256: D = 2048, and (ImageNet stem on 64 x 64 images:
    a 2 x 2 last map) a feature row that comes from torch's pooling, not from the fused 4 x 4
    pool: bitwise the same rows, logits and scores whatever the launch chunk."""
    n, nc = 256, 100
    images, labels = synthetic.make_images(n, nc, seed=31, hw=64)
    sd = synthetic.make_checkpoint("resnet50", nc, seed=6, stem="imagenet")["net"]
    models = checkpoints.build_models([sd], "resnet50", nc, "imagenet", device=cuda)
    img, lab = torch.from_numpy(images).to(cuda), torch.from_numpy(labels).to(cuda)
    rec = Recorder(monkeypatch)
    out = {}
    for chunk in (128, 256):
        rec.calls.clear()
        eng = ScoringEngine(models, ScoreConfig(methods=("el2n", "proto"), el2n_chunk=chunk),
                            cuda)
        out[chunk] = eng.score_shard(img, lab, 0, n)
        assert len(rec.calls) == n // chunk
        feats = rec.features(models)
        assert feats.shape == (1, n, 2048)
        out[chunk, "feat"] = feats
    assert np.array_equal(out[128, "feat"], out[256, "feat"])
    for m in ("el2n", "proto"):
        assert torch.equal(out[128][m], out[256][m]), m
    check_proto(out[128]["proto"], out[128, "feat"], labels, nc, "resnet50")


def test_selection_by_proto(cuda, case):
    eng = engine(case, cuda, ("el2n", "proto"), select_by="proto")
    full, kept, k = eng.run(case["img"], case["lab"], 0.6)
    assert torch.equal(kept, _capi.select_topk(full["proto"], k)[0])
    assert eng.last_refine is None
    eng = engine(case, cuda, ("el2n", "proto"), select_by="proto", select_policy="balanced")
    full_b, kept, k = eng.run(case["img"], case["lab"], 0.6)
    assert torch.equal(full_b["proto"], full["proto"])
    want = ref_select(full_b["proto"].cpu().numpy(), case["labels"], C, k, "balanced")
    assert np.array_equal(kept.cpu().numpy(), want)


def test_proto_alone_and_its_label_check(cuda, case):
    eng = engine(case, cuda, ("proto",))
    full, kept, k = eng.run(case["img"], case["lab"], 0.5)
    assert list(full) == ["proto"] and k == 150
    both = engine(case, cuda, ("el2n", "proto")).run(case["img"], case["lab"], 0.5)[0]
    assert torch.equal(full["proto"], both["proto"])
    lab = case["lab"].clone()
    lab[280] = C  # in the ragged last batch
    with pytest.raises(_capi.LabelError, match="1 label"):
        eng.run(case["img"], lab, 0.5)
    with pytest.raises(_capi.LabelError):
        eng.score_shard(case["img"], lab, 256, 300)


def test_fp16_overflow_rescores_proto_with_the_family(cuda):
    """The checkpoint of test_fp16_overflow_rescores_the_whole_family: a non-finite feature
    poisons its class's centroid, score_shard raises, run() falls back to bf16 halves for the
    whole family and proto is bitwise an engine built on bf16 packs."""
    n = 256
    images, labels = synthetic.make_images(n, C, seed=9)
    sd = synthetic.make_checkpoint("resnet18", C, seed=4)["net"]
    sd["layer1.0.bn1.weight"] = sd["layer1.0.bn1.weight"] * 1e5
    img, lab = torch.from_numpy(images).to(cuda), torch.from_numpy(labels).to(cuda)
    methods = ("el2n", "proto")
    cfg = dict(methods=methods, select_by="proto")
    eng = ScoringEngine(checkpoints.build_models([sd], device=cuda), ScoreConfig(**cfg), cuda)
    with pytest.raises(ValueError, match="non-finite"):
        eng.score_shard(img, lab, 0, n)
    full, kept, k = eng.run(img, lab, 0.5)
    assert set(eng.fallback) == set(methods) and eng.cfg.el2n_operands == "bf16x3"
    assert eng.cfg.methods == methods
    ref = ScoringEngine(checkpoints.build_models([sd], device=cuda),
                        ScoreConfig(el2n_operands="bf16x3", **cfg), cuda)
    full_r, kept_r, _ = ref.run(img, lab, 0.5)
    assert ref.fallback == {}
    for m in methods:
        assert bool(torch.isfinite(full[m]).all()) and torch.equal(full[m], full_r[m]), m
    assert torch.equal(kept, kept_r)


def test_outer_layers(cuda, case, tmp_path):
    from data_diet_distributed_amd.resnet import ResNet18
    net = ResNet18().to(cuda)
    net.load_state_dict(case["sds"][0])
    ds = MyDataset(ArrayImageDataset(case["images"], case["labels"]))
    loader = torch.utils.data.DataLoader(ds, batch_size=128, shuffle=False)
    with pytest.raises(ValueError, match="engine"):
        sparse_loader(loader, N, net, cuda, 0.5, 128, 0, score="proto")
    # the config entry: score_methods / select_by reach the engine and the artefact's metadata
    ck = tmp_path / "checkpoint"
    os.makedirs(ck)
    torch.save({"net": case["sds"][0], "acc": 0.0, "epoch": 19}, ck / "ckpt_19.pth")
    (tmp_path / "p.yaml").write_text(
        f"dataset: synthetic-cifar10\nsynthetic_n: {N}\nsynthetic_seed: 57\nbatch_size: 128\n"
        f"sparsity: 0.5\ncheckpoint_path: {ck}\nscore_methods: [el2n, proto]\n"
        f"select_by: proto\n")
    out = str(tmp_path / "idx" / "proto")
    assert score.main(["--config", str(tmp_path / "p.yaml"), "--out", out]) == 0
    idx, meta = subset_index.read_subset_index(out)
    assert meta["score_methods"] == ["el2n", "proto"] and meta["select_by"] == "proto"
    assert meta["k"] == 150 and len(idx) == 150


def test_two_ranks_equal_world1_bitwise(cuda, tmp_path):
    """Two rank processes on cuda:0 over gloo, each holding only its shard: the class means
    span both shards through the exact int64 all-reduce, so the gathered proto vector and the
    keep-set equal the single-process run bit for bit, in at most K + 1 all-reduces."""
    from data_diet_distributed_amd import launch
    from helpers import proto_child
    n = 2 * 1024 + 3 * 128 + 40  # shards [0, 1280), [1280, 2472): chunk plans differ per rank
    out = str(tmp_path / "w2.npz")
    assert launch.launch_ranks(2, [os.path.abspath(proto_child.__file__), out, str(n)]) == 0
    w2 = np.load(out)
    assert int(w2["world"]) == 2 and str(w2["backend"]) == "gloo"
    assert w2["shard"].tolist() == list(shard_bounds(n, 128, 2, 0))
    assert int(w2["all_reduce"]) <= len(proto_child.CKPT_SEEDS) + 1 and int(w2["fallback"]) == 0
    images, labels = synthetic.make_images(n, 10, seed=proto_child.DATA_SEED)
    sds = [synthetic.make_checkpoint("resnet18", 10, seed=s)["net"]
           for s in proto_child.CKPT_SEEDS]
    eng = ScoringEngine(checkpoints.build_models(sds, device=cuda),
                        ScoreConfig(methods=("el2n", "proto"), select_by="proto"), cuda)
    full, kept, k = eng.run(torch.from_numpy(images).to(cuda), torch.from_numpy(labels).to(cuda),
                            0.5)
    for m in ("el2n", "proto"):
        got, want = w2[m], full[m].cpu().numpy()
        assert np.array_equal(got, want), (m, float(np.max(np.abs(got / want - 1))))
    assert int(w2["k"]) == k and np.array_equal(w2["kept"], kept.cpu().numpy())
