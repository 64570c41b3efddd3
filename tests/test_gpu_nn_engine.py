"""The nearest-same-class-neighbour score through the product layers: ScoringEngine (the shared
feature buffer, the second phase of a checkpoint, chunk sizes, lanes, shards, the general path,
ResNet-50, selection, a planted duplicate, the singleton-class error, two ranks), sparse_loader
and the config entry.  The case of tests/test_gpu_proto_engine.py: ResNet-18, K = 3 synthetic
checkpoints, N = 300 = two full batches of 128 + a ragged 44, 10 classes, el2n_chunk = 128.
Scores are compared with the NumPy restatement (tests/test_nn_scores.py) applied to the feature
rows the run itself produced, recorded by wrapping the forward.
"""
import os

import numpy as np
import pytest
import torch

from data_diet_distributed_amd import _capi, checkpoints, el2n_fast, forward_scores, score
from data_diet_distributed_amd import scoring, subset_index, synthetic
from data_diet_distributed_amd.get_scores_and_prune import sparse_loader
from data_diet_distributed_amd.loader import ArrayImageDataset, MyDataset
from data_diet_distributed_amd.resnet import ResNet
from data_diet_distributed_amd.scoring import ScoreConfig, ScoringEngine, shard_bounds
from test_nn_scores import pick_bound, ref_nn, value_bound
from test_select_policy import ref_select

pytestmark = pytest.mark.gpu

N, C, K = 300, 10, 3
DUP = (5, 77)  # the planted duplicate: two positions of one BN batch, so their rows are equal


@pytest.fixture(scope="module")
def case(cuda):
    images, labels = synthetic.make_images(N, C, seed=57)
    sds = [synthetic.make_checkpoint("resnet18", C, seed=s)["net"] for s in (11, 12, 13)]
    return {"images": images, "labels": labels, "sds": sds,
            "models": checkpoints.build_models(sds, device=cuda),
            "img": torch.from_numpy(images).to(cuda), "lab": torch.from_numpy(labels).to(cuda)}


@pytest.fixture(scope="module")
def dup_case(case, cuda):
    """The case with image DUP[0] copied over DUP[1] (label too)."""
    images, labels = case["images"].copy(), case["labels"].copy()
    images[DUP[1]], labels[DUP[1]] = images[DUP[0]], labels[DUP[0]]
    assert np.bincount(labels, minlength=C).min() >= 2
    return {"images": images, "labels": labels,
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


def check_nn(got, feature_sets, labels, num_classes, operands="f16x3", what=""):
    """The engine's nn vector against the restatement on `feature_sets` [K, n, D]: not below the
    true nearest distance less the value bound, and not above the mean over the checkpoints of
    the farthest distance the pick bound admits."""
    Kc, _, D = feature_sets.shape
    assert feature_sets.dtype == np.float32
    ref = ref_nn(feature_sets, labels, num_classes)[0]
    upper = np.zeros_like(ref)
    for f in feature_sets:
        one = ref_nn(f[None], labels, num_classes)[0]
        upper += np.sqrt(one ** 2 + pick_bound(f, labels, operands))
    upper /= Kc
    got = got.cpu().numpy().astype(np.float64)
    lower = ref * (1 - value_bound(D))
    print(f"nn {what}: D={D} K={Kc} got/ref - 1 in [{(got / ref - 1).min():.3g}, "
          f"{(got / ref - 1).max():.3g}], value bound {value_bound(D):.3g}, "
          f"upper/ref - 1 >= {(upper / ref - 1).min():.3g}; scores {ref.min():.3g} .. "
          f"{ref.max():.3g}")
    assert np.all(np.isfinite(ref)) and ref.max() > 0
    assert np.all(got >= lower) and np.all(got <= upper)


def test_nn_against_recorded_features(cuda, case, monkeypatch):
    methods = scoring.LOGIT_FAMILY + ("proto", "nn", "grand")
    before = engine(case, cuda, ("el2n", "proto")).run(case["img"], case["lab"], 0.5)[0]
    rec = Recorder(monkeypatch)
    full, kept, k = engine(case, cuda, methods).run(case["img"], case["lab"], 0.5)
    assert set(full) == set(methods) and all(v.numel() == N for v in full.values())
    assert len(rec.calls) == K * 3  # still one forward per checkpoint and chunk
    for m in ("el2n", "proto"):  # bitwise unchanged by adding nn
        assert torch.equal(full[m], before[m]), m
    assert all(bool(torch.isfinite(v).all()) for v in full.values())
    feats = rec.features(case["models"])
    assert feats.shape == (K, N, 512)
    check_nn(full["nn"], feats, case["labels"], C, what="resnet18")


def test_nn_is_bitwise_invariant(cuda, case, monkeypatch):
    """The chunk size, lanes and concurrent passes change no bit; nor does the split of the
    queries over shards, each searching the whole set's rows (a fake gather hands every shard
    the rows the one-rank run produced)."""
    img, lab = case["img"], case["lab"]
    methods = ("el2n", "proto", "nn")
    saved = []
    inner = scoring.gather_rows

    def recording(t, lengths, group=None):
        if t.dim() == 2:
            saved.append(t.clone())
        return inner(t, lengths, group)

    monkeypatch.setattr(forward_scores, "gather_rows", recording)
    one = engine(case, cuda, methods).score_shard(img, lab, 0, N)
    monkeypatch.setattr(forward_scores, "gather_rows", inner)
    assert len(saved) == K
    for kw in ({"el2n_chunk": 256}, {"el2n_chunk": 1024}, {"lanes": 2},
               {"lanes": 2, "el2n_chunk": 256}):
        got = engine(case, cuda, methods, **kw).score_shard(img, lab, 0, N)
        for m in methods:
            assert torch.equal(got[m], one[m]), (kw, m)
    both = methods + ("grand",)
    conc = engine(case, cuda, both, concurrent_passes=True).score_shard(img, lab, 0, N)
    for m in methods:
        assert torch.equal(conc[m], one[m]), m
    alone = engine(case, cuda, ("nn",)).score_shard(img, lab, 0, N)
    assert torch.equal(alone["nn"], one["nn"])
    # a direct shard call without a group searches the shard only
    part = engine(case, cuda, ("nn",)).score_shard(img, lab, 0, 256)
    assert not torch.equal(part["nn"], one["nn"][:256])
    assert bool((part["nn"] >= one["nn"][:256]).all())  # fewer candidates: never nearer
    for W in (2, 3):
        bounds = [shard_bounds(N, 128, W, r) for r in range(W)]
        for r, (lo, hi) in enumerate(bounds):
            turn = iter(saved)
            monkeypatch.setattr(forward_scores, "shard_lengths",
                                lambda n, group=None: ([b - a for a, b in bounds], r))
            monkeypatch.setattr(forward_scores, "gather_rows", lambda t, lengths, group=None: (
                lab if t.dim() == 1 else next(turn)))
            got = engine(case, cuda, ("el2n", "nn")).score_shard(img, lab, lo, hi)
            assert torch.equal(got["nn"], one["nn"][lo:hi]), (W, r)
            assert torch.equal(got["el2n"], one["el2n"][lo:hi]), (W, r)


@pytest.mark.parametrize("kw", [{"fast_el2n": False}, {"el2n_operands": "bf16x3"}],
                         ids=["fast_el2n_off", "bf16_halves"])
def test_general_path_and_bf16_halves(cuda, case, monkeypatch, kw):
    """model.run per batch (no grouped forward): the features are the classifier's input rows on
    that path's tape, again from one forward per checkpoint and batch; and the grouped forward
    on bf16 halves, whose wider pick bound applies."""
    if "fast_el2n" in kw:
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
        sets = lambda: np.stack([np.concatenate([f for mid, f in calls if mid == id(m)])  # noqa
                                 for m in case["models"]])
    else:
        rec = Recorder(monkeypatch)
        calls = rec.calls
        sets = lambda: rec.features(case["models"])  # noqa: E731
    full = engine(case, cuda, ("el2n", "nn"), **kw).score_shard(case["img"], case["lab"], 0, N)
    assert len(calls) == K * 3
    feats = sets()
    assert feats.shape == (K, N, 512)
    check_nn(full["nn"], feats, case["labels"], C, kw.get("el2n_operands", "f16x3"), str(kw))


def test_resnet50_wide_features(cuda, monkeypatch):
    """ResNet-50 (ImageNet stem on 64 x 64 images), K = 1, N = 130 = one full batch and a ragged
    2, D = 2048: bitwise the same over two chunk sizes, and within the bounds."""
    n, nc = 130, 10
    images, labels = synthetic.make_images(n, nc, seed=31, hw=64)
    assert np.bincount(labels, minlength=nc).min() >= 2
    sd = synthetic.make_checkpoint("resnet50", nc, seed=6, stem="imagenet")["net"]
    models = checkpoints.build_models([sd], "resnet50", nc, "imagenet", device=cuda)
    img, lab = torch.from_numpy(images).to(cuda), torch.from_numpy(labels).to(cuda)
    rec = Recorder(monkeypatch)
    out = {}
    for chunk in (128, 256):
        rec.calls.clear()
        eng = ScoringEngine(models, ScoreConfig(methods=("el2n", "nn"), el2n_chunk=chunk), cuda)
        out[chunk] = eng.score_shard(img, lab, 0, n)
        out[chunk, "feat"] = rec.features(models)
        assert out[chunk, "feat"].shape == (1, n, 2048)
    for m in ("el2n", "nn"):
        assert torch.equal(out[128][m], out[256][m]), m
    check_nn(out[128]["nn"], out[128, "feat"], labels, nc, what="resnet50")


def test_selection_by_nn(cuda, case):
    eng = engine(case, cuda, ("el2n", "nn"), select_by="nn")
    full, kept, k = eng.run(case["img"], case["lab"], 0.6)
    assert torch.equal(kept, _capi.select_topk(full["nn"], k)[0])
    assert eng.last_refine is None
    eng = engine(case, cuda, ("el2n", "nn"), select_by="nn", select_policy="balanced")
    full_b, kept, k = eng.run(case["img"], case["lab"], 0.6)
    assert torch.equal(full_b["nn"], full["nn"])
    want = ref_select(full_b["nn"].cpu().numpy(), case["labels"], C, k, "balanced")
    assert np.array_equal(kept.cpu().numpy(), want)


def test_planted_duplicate_scores_lowest_and_is_dropped(cuda, case, dup_case):
    eng = engine(case, cuda, ("nn",))
    full, kept, k = eng.run(dup_case["img"], dup_case["lab"], 0.5)
    s = full["nn"].cpu().numpy()
    others = np.delete(s, DUP)
    assert s[DUP[0]] == 0.0 and s[DUP[1]] == 0.0 and others.min() > 0
    assert k == 150 and not np.isin(DUP, kept.cpu().numpy()).any()


def test_singleton_class_raises_by_name(cuda, case):
    lab = case["lab"].clone()
    members = torch.nonzero(lab == 9).flatten()
    lab[members[1:]] = 0  # class 9 keeps exactly one member
    eng = engine(case, cuda, ("el2n", "nn"))
    with pytest.raises(ValueError, match="class 9 has exactly one member"):
        eng.run(case["img"], lab, 0.5)
    with pytest.raises(ValueError, match="class 9"):
        eng.score_shard(case["img"], lab, 0, N)
    lab[int(members[0])] = C  # ... and a label outside [0, C) is still a LabelError
    with pytest.raises(_capi.LabelError, match="1 label"):
        engine(case, cuda, ("nn",)).run(case["img"], lab, 0.5)


@pytest.mark.parametrize("methods", [("nn",), ("proto", "nn"), ("loss", "proto", "nn"),
                                     ("el2n", "loss"), ("grand", "nn"), ("nn", "grand")],
                         ids=lambda m: "+".join(m))
def test_each_bad_label_is_counted_once(cuda, case, methods):
    """One label outside [0, C) among 130 rows (a full batch and a ragged 2) over K = 3
    checkpoints is reported as one label, whichever kernel or class count does the counting:
    not once per checkpoint, per pass or per requested score."""
    lab = case["lab"].clone()
    counts = torch.bincount(lab[:130], minlength=C)
    row = int(torch.nonzero(lab[:130] == int(counts.argmax()))[0])
    assert int(counts.max()) >= 3  # the class keeps at least two members: no singleton
    lab[row] = C
    with pytest.raises(_capi.LabelError, match="1 label"):
        engine(case, cuda, methods).score_shard(case["img"], lab, 0, 130)


def test_outer_layers(cuda, case, dup_case, tmp_path):
    from data_diet_distributed_amd.resnet import ResNet18
    net = ResNet18().to(cuda)
    net.load_state_dict(case["sds"][0])
    ds = MyDataset(ArrayImageDataset(dup_case["images"], dup_case["labels"]))
    loader = torch.utils.data.DataLoader(ds, batch_size=128, shuffle=False)
    for fast in (True, False):
        _, samples, idx = sparse_loader(loader, N, net, cuda, 0.5, 128, 0, score="nn",
                                        fast=fast, return_indices=True)
        assert sparse_loader.last_path == ("fast" if fast else "general")
        assert samples == 150 and len(set(idx)) == 150
        assert not set(DUP) & set(idx)  # the duplicate pair scores 0: dropped first
    with pytest.raises(ValueError, match="refine"):
        sparse_loader(loader, N, net, cuda, 0.5, 128, 0, score="nn", refine=True)
    # the config entry: score_methods / select_by reach the engine and the artefact's metadata
    ck = tmp_path / "checkpoint"
    os.makedirs(ck)
    torch.save({"net": case["sds"][0], "acc": 0.0, "epoch": 19}, ck / "ckpt_19.pth")
    (tmp_path / "p.yaml").write_text(
        f"dataset: synthetic-cifar10\nsynthetic_n: {N}\nsynthetic_seed: 57\nbatch_size: 128\n"
        f"sparsity: 0.5\ncheckpoint_path: {ck}\nscore_methods: [el2n, nn]\n"
        f"select_by: nn\n")
    out = str(tmp_path / "idx" / "nn")
    assert score.main(["--config", str(tmp_path / "p.yaml"), "--out", out]) == 0
    idx, meta = subset_index.read_subset_index(out)
    assert meta["score_methods"] == ["el2n", "nn"] and meta["select_by"] == "nn"
    assert meta["k"] == 150 and len(idx) == 150


def test_two_ranks_equal_world1_bitwise(cuda, tmp_path):
    """Two rank processes on cuda:0 over gloo, each holding only its shard: every rank searches
    its rows among both shards' rows, so the gathered nn vector and the keep-set equal the
    single-process run bit for bit."""
    from data_diet_distributed_amd import launch
    from helpers import nn_child
    n = 2 * 1024 + 3 * 128 + 40  # shards [0, 1280), [1280, 2472): chunk plans differ per rank
    out = str(tmp_path / "w2.npz")
    assert launch.launch_ranks(2, [os.path.abspath(nn_child.__file__), out, str(n)]) == 0
    w2 = np.load(out)
    assert int(w2["world"]) == 2 and str(w2["backend"]) == "gloo"
    assert w2["shard"].tolist() == list(shard_bounds(n, 128, 2, 0))
    assert int(w2["all_gather"]) <= nn_child.MAX_GATHERS and int(w2["fallback"]) == 0
    images, labels = synthetic.make_images(n, 10, seed=nn_child.DATA_SEED)
    sds = [synthetic.make_checkpoint("resnet18", 10, seed=s)["net"]
           for s in nn_child.CKPT_SEEDS]
    eng = ScoringEngine(checkpoints.build_models(sds, device=cuda),
                        ScoreConfig(methods=nn_child.METHODS, select_by="nn"), cuda)
    full, kept, k = eng.run(torch.from_numpy(images).to(cuda), torch.from_numpy(labels).to(cuda),
                            0.5)
    for m in nn_child.METHODS:
        got, want = w2[m], full[m].cpu().numpy()
        assert np.array_equal(got, want), (m, float(np.max(np.abs(got / want - 1))))
    assert int(w2["k"]) == k and np.array_equal(w2["kept"], kept.cpu().numpy())
