"""The knn scores through the product layers: ScoringEngine (the shared feature buffer and the one
all-gather of the rows shared with nn, chunk sizes, lanes, shards, the general path, bf16 halves,
ResNet-50, the small-dataset error, the label count, two ranks), sparse_loader and the config
entry.  The case of tests/test_gpu_nn_engine.py: ResNet-18, K = 3 synthetic checkpoints, N = 300 =
two full batches of 128 + a ragged 44, 10 classes, el2n_chunk = 128.  Scores are compared with
the NumPy restatement (tests/test_knn_scores.py) applied to the feature rows the run itself
produced, recorded by wrapping the forward.

The bounds on the engine's vectors, from those of tests/test_knn_scores.py.  Per checkpoint let
T_1 <= ... <= T_k be the true k smallest squared distances of a row.  At least i keys are at most
T_i + e (e = half the pick bound, the error of one key), so the i-th pick in key order has a key
of at most T_i + e and a true squared distance of at most T_i + 2 e; and no k rows have a smaller
sum of distances than the true neighbours.  Hence
    mean_i sqrt(T_i)  <=  knn  <=  mean_i sqrt(T_i + pick bound),
each side widened by the value bound, then averaged over the checkpoints.  knn_disagree is
compared where the gap is above the floor in EVERY checkpoint: there the sets are the
reference's, and K fp32 additions of shares in [0, 1] and one division differ from the float64
mean by at most (K + 2) 2^-23.
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
from test_knn_scores import gap_floor, pick_bound, ref_knn, sq_dists
from test_nn_scores import value_bound

pytestmark = pytest.mark.gpu

N, C, K = 300, 10, 3
KNN = ("knn", "knn_disagree")


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


def check_knn(full, feature_sets, labels, k, operands="f16x3", what=""):
    """The engine's knn / knn_disagree vectors against the restatement on `feature_sets`
    [K, n, D], within the bounds of the module docstring."""
    Kc, n, D = feature_sets.shape
    assert feature_sets.dtype == np.float32
    lower, upper, share = np.zeros(n), np.zeros(n), np.zeros(n)
    clear = np.ones(n, bool)
    for f in feature_sets:
        nbrs, _, dis, gap = ref_knn(f[None], labels, k)
        true = np.take_along_axis(sq_dists(f), nbrs[0], axis=1)
        lower += np.sqrt(true).mean(axis=1)
        upper += np.sqrt(true + pick_bound(f, operands)[:, None]).mean(axis=1)
        share += dis
        clear &= gap[0] > gap_floor(f)
    lower, upper, share = lower / Kc, upper / Kc, share / Kc
    vb = value_bound(D)
    got = full["knn"].cpu().numpy().astype(np.float64)
    print(f"knn {what}: D={D} K={Kc} k={k} got/ref - 1 in [{(got / lower - 1).min():.3g}, "
          f"{(got / lower - 1).max():.3g}], value bound {vb:.3g}, upper/ref - 1 >= "
          f"{(upper / lower - 1).min():.3g}; scores {lower.min():.3g} .. {lower.max():.3g}; "
          f"{100 * clear.mean():.1f} % of the rows above the gap floor in every checkpoint")
    assert np.all(np.isfinite(lower)) and lower.max() > 0
    assert np.all(got >= lower * (1 - vb)) and np.all(got <= upper * (1 + vb))
    dis = full["knn_disagree"].cpu().numpy().astype(np.float64)
    assert np.all((dis >= 0) & (dis <= 1)) and clear.any()
    assert np.all(np.abs(dis[clear] - share[clear]) <= (Kc + 2) * 2.0 ** -23)


def test_knn_against_recorded_features(cuda, case, monkeypatch):
    methods = scoring.LOGIT_FAMILY + ("proto", "nn") + KNN + ("grand",)
    before = engine(case, cuda, ("el2n", "proto", "nn")).run(case["img"], case["lab"], 0.5)[0]
    rec = Recorder(monkeypatch)
    full, kept, k = engine(case, cuda, methods).run(case["img"], case["lab"], 0.5)
    assert set(full) == set(methods) and all(v.numel() == N for v in full.values())
    assert len(rec.calls) == K * 3  # still one forward per checkpoint and chunk
    for m in ("el2n", "proto", "nn"):  # bitwise unchanged by adding the knn scores
        assert torch.equal(full[m], before[m]), m
    assert all(bool(torch.isfinite(v).all()) for v in full.values())
    feats = rec.features(case["models"])
    assert feats.shape == (K, N, 512)
    check_knn(full, feats, case["labels"], 5, what="resnet18")
    # another k, one score alone, selection by it
    eng = engine(case, cuda, ("knn_disagree",), knn_k=16)
    alone, kept, k = eng.run(case["img"], case["lab"], 0.6)
    assert torch.equal(kept, _capi.select_topk(alone["knn_disagree"], k)[0])
    assert eng.last_refine is None
    both = engine(case, cuda, KNN, knn_k=16).score_shard(case["img"], case["lab"], 0, N)
    assert torch.equal(both["knn_disagree"], alone["knn_disagree"])
    check_knn(both, feats, case["labels"], 16, what="resnet18 k=16")


def test_knn_is_bitwise_invariant(cuda, case, monkeypatch):
    """The chunk size, lanes and concurrent passes change no bit; nor does the split of the
    queries over shards, each searching the whole set's rows (a fake gather hands every shard
    the rows the one-rank run produced).  nn and the knn scores share ONE gather of the rows per
    checkpoint."""
    img, lab = case["img"], case["lab"]
    methods = ("el2n", "proto", "nn") + KNN
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
    alone = engine(case, cuda, KNN).score_shard(img, lab, 0, N)
    for m in KNN:
        assert torch.equal(alone[m], one[m]), m
    # a direct shard call without a group searches the shard only
    part = engine(case, cuda, ("knn",)).score_shard(img, lab, 0, 256)
    assert not torch.equal(part["knn"], one["knn"][:256])
    assert bool((part["knn"] >= one["knn"][:256]).all())  # fewer candidates: never nearer
    for W in (2, 3):
        bounds = [shard_bounds(N, 128, W, r) for r in range(W)]
        for r, (lo, hi) in enumerate(bounds):
            turn = iter(saved)
            monkeypatch.setattr(forward_scores, "shard_lengths",
                                lambda n, group=None: ([b - a for a, b in bounds], r))
            monkeypatch.setattr(forward_scores, "gather_rows", lambda t, lengths, group=None: (
                lab if t.dim() == 1 else next(turn)))
            got = engine(case, cuda, ("el2n", "nn") + KNN).score_shard(img, lab, lo, hi)
            for m in ("el2n", "nn") + KNN:
                assert torch.equal(got[m], one[m][lo:hi]), (W, r, m)


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
    full = engine(case, cuda, ("el2n",) + KNN, **kw).score_shard(case["img"], case["lab"], 0, N)
    assert len(calls) == K * 3
    feats = sets()
    assert feats.shape == (K, N, 512)
    check_knn(full, feats, case["labels"], 5, kw.get("el2n_operands", "f16x3"), str(kw))


def test_resnet50_wide_features(cuda, monkeypatch):
    """ResNet-50 (ImageNet stem on 64 x 64 images), K = 1, N = 130 = one full batch and a ragged
    2, D = 2048: bitwise the same over two chunk sizes, and within the bounds."""
    n, nc = 130, 10
    images, labels = synthetic.make_images(n, nc, seed=31, hw=64)
    sd = synthetic.make_checkpoint("resnet50", nc, seed=6, stem="imagenet")["net"]
    models = checkpoints.build_models([sd], "resnet50", nc, "imagenet", device=cuda)
    img, lab = torch.from_numpy(images).to(cuda), torch.from_numpy(labels).to(cuda)
    rec = Recorder(monkeypatch)
    out = {}
    for chunk in (128, 256):
        rec.calls.clear()
        eng = ScoringEngine(models, ScoreConfig(methods=("el2n",) + KNN, el2n_chunk=chunk), cuda)
        out[chunk] = eng.score_shard(img, lab, 0, n)
        out[chunk, "feat"] = rec.features(models)
        assert out[chunk, "feat"].shape == (1, n, 2048)
    for m in ("el2n",) + KNN:
        assert torch.equal(out[128][m], out[256][m]), m
    check_knn(out[128], out[128, "feat"], labels, 5, what="resnet50")


def test_small_dataset_raises_by_name(cuda, case):
    eng = engine(case, cuda, ("el2n", "knn"), knn_k=16)
    with pytest.raises(ValueError, match="knn_k=16"):
        eng.score_shard(case["img"], case["lab"], 0, 16)
    with pytest.raises(ValueError, match="knn_k=16"):
        eng.run(case["img"][:16], case["lab"][:16], 0.5)
    out = eng.score_shard(case["img"], case["lab"], 0, 17)  # 16 other rows: enough
    assert bool(torch.isfinite(out["knn"]).all())


@pytest.mark.parametrize("methods", [("knn",), ("knn_disagree", "nn"), ("proto", "knn"),
                                     ("loss", "knn_disagree"), ("grand", "knn"),
                                     ("knn", "grand")], ids=lambda m: "+".join(m))
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


def test_outer_layers(cuda, case, tmp_path, monkeypatch):
    from data_diet_distributed_amd.resnet import ResNet18
    net = ResNet18().to(cuda)
    net.load_state_dict(case["sds"][0])
    ds = MyDataset(ArrayImageDataset(case["images"], case["labels"]))
    loader = torch.utils.data.DataLoader(ds, batch_size=128, shuffle=False)
    seen = []
    inner = forward_scores.nearest_k

    def recording(features, labels, num_classes, k, operands="f16x3"):
        out = inner(features, labels, num_classes, k, operands)
        seen.append((features.cpu().numpy().copy(), labels.cpu().numpy().copy(), k,
                     [t.cpu().numpy().copy() for t in out]))
        return out

    monkeypatch.setattr(forward_scores, "nearest_k", recording)
    for fast in (True, False):
        for which, name in enumerate(KNN):
            seen.clear()
            _, samples, idx = sparse_loader(loader, N, net, cuda, 0.5, 128, 0, score=name,
                                            fast=fast, return_indices=True, knn_k=7)
            assert sparse_loader.last_path == ("fast" if fast else "general")
            assert samples == 150 and len(set(idx)) == 150 and len(seen) == 1
            feats, labels, k, scores = seen[0]
            assert k == 7 and feats.shape == (N, 512) and np.array_equal(labels, case["labels"])
            # the visit order is the dataset's: the keep-set is the top half by that score
            want = _capi.select_topk(torch.from_numpy(scores[which]).to(cuda), 150)[0]
            assert idx == want.cpu().tolist()
            full = {m: torch.from_numpy(s) for m, s in zip(KNN, scores)}
            check_knn(full, feats[None], labels, 7, what=f"sparse_loader fast={fast}")
    with pytest.raises(ValueError, match="refine"):
        sparse_loader(loader, N, net, cuda, 0.5, 128, 0, score="knn", refine=True)
    # the config entry: score_methods / select_by / knn_k reach the engine and the metadata
    ck = tmp_path / "checkpoint"
    os.makedirs(ck)
    torch.save({"net": case["sds"][0], "acc": 0.0, "epoch": 19}, ck / "ckpt_19.pth")
    (tmp_path / "p.yaml").write_text(
        f"dataset: synthetic-cifar10\nsynthetic_n: {N}\nsynthetic_seed: 57\nbatch_size: 128\n"
        f"sparsity: 0.5\ncheckpoint_path: {ck}\nscore_methods: [el2n, knn, knn_disagree]\n"
        f"select_by: knn\nknn_k: 7\n")
    out = str(tmp_path / "idx" / "knn")
    assert score.main(["--config", str(tmp_path / "p.yaml"), "--out", out]) == 0
    idx, meta = subset_index.read_subset_index(out)
    assert meta["score_methods"] == ["el2n", "knn", "knn_disagree"] and meta["select_by"] == "knn"
    assert meta["k"] == 150 and len(idx) == 150 and meta["knn_k"] == 7


def test_two_ranks_equal_world1_bitwise(cuda, tmp_path):
    """Two rank processes on cuda:0 over gloo, each holding only its shard: every rank searches
    its rows among both shards' rows, so the gathered vectors and the keep-set equal the
    single-process run bit for bit; nn and the knn scores share the gathers."""
    from data_diet_distributed_amd import launch
    from helpers import knn_child
    n = 2 * 1024 + 3 * 128 + 40  # shards [0, 1280), [1280, 2472): chunk plans differ per rank
    out = str(tmp_path / "w2.npz")
    assert launch.launch_ranks(2, [os.path.abspath(knn_child.__file__), out, str(n)]) == 0
    w2 = np.load(out)
    assert int(w2["world"]) == 2 and str(w2["backend"]) == "gloo"
    assert w2["shard"].tolist() == list(shard_bounds(n, 128, 2, 0))
    assert int(w2["all_gather"]) <= knn_child.MAX_GATHERS and int(w2["fallback"]) == 0
    images, labels = synthetic.make_images(n, 10, seed=knn_child.DATA_SEED)
    sds = [synthetic.make_checkpoint("resnet18", 10, seed=s)["net"]
           for s in knn_child.CKPT_SEEDS]
    eng = ScoringEngine(checkpoints.build_models(sds, device=cuda),
                        ScoreConfig(methods=knn_child.METHODS, select_by="knn"), cuda)
    full, kept, k = eng.run(torch.from_numpy(images).to(cuda), torch.from_numpy(labels).to(cuda),
                            0.5)
    for m in knn_child.METHODS:
        got, want = w2[m], full[m].cpu().numpy()
        assert np.array_equal(got, want), (m, float(np.max(np.abs(got - want))))
    assert int(w2["k"]) == k and np.array_equal(w2["kept"], kept.cpu().numpy())
