"""The logit-score family through the product layers: ScoringEngine (one shared forward per
checkpoint, lanes, shards, the general path, selection) and sparse_loader (ResNet-18, K = 3
synthetic checkpoints, N = 300 = two full batches of 128 + a ragged 44, 10 classes).  Scores are
compared with the NumPy restatement (tests/test_logit_scores.py) applied to the logits the run
itself produced, recorded by wrapping the forward.
"""
import numpy as np
import pytest
import torch

from data_diet_distributed_amd import _capi, checkpoints, el2n_fast, subset_index, synthetic
from data_diet_distributed_amd.get_scores_and_prune import sparse_loader
from data_diet_distributed_amd.loader import ArrayImageDataset, MyDataset
from data_diet_distributed_amd.resnet import ResNet
from data_diet_distributed_amd.scoring import (LOGIT_FAMILY, LOGIT_METHODS, ScoreConfig,
                                               ScoringEngine)
from test_logit_scores import ATOL, RTOL, STATS, ref_ensemble, ref_logit_stats
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
    """Wraps el2n_fast.forward_logits: counts the calls and keeps each call's valid logits."""

    def __init__(self, monkeypatch):
        self.calls = []
        inner = el2n_fast.forward_logits

        def wrapped(model, x, group_size, n_valid):
            out = inner(model, x, group_size, n_valid)
            self.calls.append((id(model), out[:n_valid].cpu().numpy().copy()))
            return out

        monkeypatch.setattr(el2n_fast, "forward_logits", wrapped)

    def logits(self, models):
        """[K, rows, C]: each model's recorded chunks in call order."""
        return np.stack([np.concatenate([z for mid, z in self.calls if mid == id(m)])
                         for m in models])


def check_against(full, logit_sets, labels, methods):
    """The engine's vectors against the restatement on `logit_sets` [K, n, C]."""
    ref = ref_ensemble(logit_sets, labels)
    Kf = np.float32(len(logit_sets))
    for m in methods:
        got = full[m].cpu().numpy()
        if m in ("margin", "error"):
            # exact given the logits: exact per-checkpoint values, the fp32 ensemble sum in
            # checkpoint order and one fp32 division (dd_ensemble_finalize)
            acc = np.zeros(len(labels), np.float32)
            for z in logit_sets:
                acc += ref_logit_stats(z, labels)[m].astype(np.float32)
            assert np.array_equal(got, acc / Kf if len(logit_sets) > 1 else acc), m
        elif m in LOGIT_METHODS:
            err = np.abs(got - ref[m]) / (ATOL + RTOL * np.abs(ref[m]))
            print(f"{m}: max error / bound = {err.max():.3g}")
            np.testing.assert_allclose(got, ref[m], rtol=RTOL, atol=ATOL, err_msg=m)


def test_whole_family_in_one_run(cuda, case, monkeypatch):
    methods = LOGIT_FAMILY + ("grand",)
    only = engine(case, cuda, ("el2n",)).run(case["img"], case["lab"], 0.5)[0]["el2n"]
    rec = Recorder(monkeypatch)
    full, kept, k = engine(case, cuda, methods).run(case["img"], case["lab"], 0.5)
    assert set(full) == set(methods) and all(v.numel() == N for v in full.values())
    assert torch.equal(full["el2n"], only)
    assert all(bool(torch.isfinite(v).all()) for v in full.values())
    check_against(full, rec.logits(case["models"]), case["labels"], LOGIT_METHODS)
    assert float(full["variability"].max()) > 0


def test_family_shares_one_forward_per_checkpoint(cuda, case, monkeypatch):
    rec = Recorder(monkeypatch)
    engine(case, cuda, ("el2n",)).run(case["img"], case["lab"], 0.5)
    alone = len(rec.calls)
    assert alone == K * 3  # three launch chunks per checkpoint
    for kw in ({}, {"lanes": 3}, {"concurrent_passes": True}):
        rec.calls.clear()
        methods = LOGIT_FAMILY + (("grand",) if kw.get("concurrent_passes") else ())
        engine(case, cuda, methods, **kw).run(case["img"], case["lab"], 0.5)
        assert len(rec.calls) == alone, kw


def test_loss_alone_and_its_label_check(cuda, case, monkeypatch):
    rec = Recorder(monkeypatch)
    eng = engine(case, cuda, ("loss",))
    full, kept, k = eng.run(case["img"], case["lab"], 0.5)
    assert list(full) == ["loss"] and k == 150
    check_against(full, rec.logits(case["models"]), case["labels"], ("loss",))
    assert torch.equal(kept, _capi.select_topk(full["loss"], k)[0])
    lab = case["lab"].clone()
    lab[280] = C  # in the ragged last batch
    with pytest.raises(_capi.LabelError, match="1 label"):
        eng.run(case["img"], lab, 0.5)
    with pytest.raises(_capi.LabelError):
        eng.score_shard(case["img"], lab, 256, 300)
    eng.score_shard(case["img"], lab, 0, 256)  # the bad row is not in [0, 256)


def test_selection_by_margin_and_class_policy(cuda, case):
    eng = engine(case, cuda, ("el2n", "margin"), select_by="margin")
    full, kept, k = eng.run(case["img"], case["lab"], 0.6)
    assert torch.equal(kept, _capi.select_topk(full["margin"], k)[0])
    assert eng.last_refine is None
    eng = engine(case, cuda, ("el2n", "margin"), select_by="margin", select_policy="balanced")
    full_b, kept, k = eng.run(case["img"], case["lab"], 0.6)
    assert torch.equal(full_b["margin"], full["margin"])
    want = ref_select(full_b["margin"].cpu().numpy(), case["labels"], C, k, "balanced")
    assert np.array_equal(kept.cpu().numpy(), want)


def test_lanes_and_shards_are_bitwise(cuda, case):
    one = engine(case, cuda, LOGIT_FAMILY).score_shard(case["img"], case["lab"], 0, N)
    eng3 = engine(case, cuda, LOGIT_FAMILY, lanes=3)
    three = eng3.score_shard(case["img"], case["lab"], 0, N)
    parts = [eng3.score_shard(case["img"], case["lab"], lo, hi) for lo, hi in ((0, 256),
                                                                               (256, 300))]
    for m in LOGIT_FAMILY:
        assert torch.equal(three[m], one[m]), m
        assert torch.equal(torch.cat([p[m] for p in parts]), one[m]), m


@pytest.mark.parametrize("kw", [{"fast_el2n": False}, {"el2n_bn": "running"}],
                         ids=["fast_el2n_off", "running_bn"])
def test_general_path(cuda, case, monkeypatch, kw):
    """model.run per batch (no grouped forward): the family is computed from that path's own
    logits, again once per checkpoint and batch."""
    calls = []
    inner = ResNet.run

    def wrapped(self, x, *a, **k):
        out = inner(self, x, *a, **k)
        nv = k.get("n_valid")
        calls.append((id(self), out[:nv if nv is not None else out.shape[0]].float().cpu()
                      .numpy().copy()))
        return out

    monkeypatch.setattr(ResNet, "run", wrapped)
    full = engine(case, cuda, LOGIT_FAMILY, **kw).score_shard(case["img"], case["lab"], 0, N)
    assert len(calls) == K * 3  # one forward per checkpoint and batch
    sets = np.stack([np.concatenate([z for mid, z in calls if mid == id(m)])
                     for m in case["models"]])
    assert sets.shape == (K, N, C)
    check_against(full, sets, case["labels"], LOGIT_METHODS)


def test_variability_and_refine_guards(cuda, case):
    with pytest.raises(ValueError, match="variability"):
        engine(case, cuda, ("el2n", "variability"), models=case["models"][:1],
               select_by="variability")
    engine(case, cuda, ("el2n", "variability"), models=case["models"][:1])  # as a by-product
    with pytest.raises(ValueError, match="refine"):
        engine(case, cuda, ("el2n", "loss"), select_by="loss", refine=True)
    shell = ScoringEngine.__new__(ScoringEngine)  # "auto" refines EL2N and GraNd only
    shell.cfg = ScoreConfig(methods=("el2n", "loss"), select_by="loss", el2n_operands="bf16x3")
    assert not shell._refines("loss") and shell._refines("el2n")


def test_fp16_overflow_rescores_the_whole_family(cuda, monkeypatch):
    """A checkpoint whose activations leave fp16's range (the BN gamma of
    test_fp16_overflow_falls_back_to_bf16_halves): every family member is non-finite on f16x3
    halves; run() rebuilds the packs on bf16 halves and re-scores the requested family in one
    forward per checkpoint and chunk again, bitwise an engine built on bf16 packs; `fallback`
    is merged into, not replaced."""
    n = 256
    images, labels = synthetic.make_images(n, C, seed=9)
    sd = synthetic.make_checkpoint("resnet18", C, seed=4)["net"]
    sd["layer1.0.bn1.weight"] = sd["layer1.0.bn1.weight"] * 1e5
    img, lab = torch.from_numpy(images).to(cuda), torch.from_numpy(labels).to(cuda)
    methods = ("loss", "el2n", "variability", "margin")
    cfg = dict(methods=methods, select_by="margin", refine=False)
    eng = ScoringEngine(checkpoints.build_models([sd], device=cuda), ScoreConfig(**cfg), cuda)
    with pytest.raises(ValueError, match="non-finite loss.*el2n_operands"):
        eng.score_shard(img, lab, 0, n)
    eng.fallback["earlier"] = "kept"
    rec = Recorder(monkeypatch)
    full, kept, k = eng.run(img, lab, 0.5)
    assert len(rec.calls) == 2  # one chunk: the f16x3 forward, then the bf16x3 one
    assert set(eng.fallback) == set(methods) | {"earlier"} and eng.grand_fallback is None
    assert eng.cfg.el2n_operands == "bf16x3" and eng.cfg.methods == methods
    ref = ScoringEngine(checkpoints.build_models([sd], device=cuda),
                        ScoreConfig(el2n_operands="bf16x3", **cfg), cuda)
    full_r, kept_r, _ = ref.run(img, lab, 0.5)
    assert ref.fallback == {}
    for m in methods:
        assert bool(torch.isfinite(full[m]).all()) and torch.equal(full[m], full_r[m]), m
    assert torch.equal(kept, kept_r)


def _loader_and_net(case, cuda):
    from data_diet_distributed_amd.resnet import ResNet18
    net = ResNet18().to(cuda)
    net.load_state_dict(case["sds"][0])  # train mode, as the reference scores
    ds = MyDataset(ArrayImageDataset(case["images"], case["labels"]))
    return torch.utils.data.DataLoader(ds, batch_size=128, shuffle=False), net


def test_sparse_loader_scores_by_loss_on_both_paths(cuda, case, monkeypatch, tmp_path):
    k = _capi.keep_count(N, 0.5)
    rec = Recorder(monkeypatch)
    for fast in (True, False):
        loader, net = _loader_and_net(case, cuda)
        outs = []
        hook = net.register_forward_hook(lambda mod, inp, out: outs.append(
            out.detach().float().cpu().numpy().copy()))
        rec.calls.clear()
        path = str(tmp_path / f"loss_{int(fast)}")
        _, samples, idx = sparse_loader(loader, N, net, cuda, 0.5, 128, 0, fast=fast,
                                        score="loss", return_indices=True,
                                        subset_index_path=path)
        hook.remove()
        assert sparse_loader.last_path == ("fast" if fast else "general")
        logits = np.concatenate([z for _, z in rec.calls] if fast else outs)
        assert logits.shape == (N, C) and samples == k
        loss = ref_logit_stats(logits, case["labels"])["loss"]
        want = np.argsort(-loss, kind="stable")[:k]
        assert sorted(idx) == sorted(want.tolist())
        meta = subset_index.read_subset_index(path)[1]
        assert meta["score_methods"] == ["loss"] and meta["select_by"] == "loss"
    loader, net = _loader_and_net(case, cuda)
    for bad in ("variability", "grand"):
        with pytest.raises(ValueError, match="engine"):
            sparse_loader(loader, N, net, cuda, 0.5, 128, 0, score=bad)
    with pytest.raises(ValueError):
        sparse_loader(loader, N, net, cuda, 0.5, 128, 0, score="foo")
    with pytest.raises(ValueError, match="refine"):
        sparse_loader(loader, N, net, cuda, 0.5, 128, 0, score="loss", refine=True)


def test_sparse_loader_default_score_is_unchanged(cuda, case, tmp_path):
    metas, kept = [], []
    for name, kw in (("default", {}), ("el2n", {"score": "el2n"})):
        loader, net = _loader_and_net(case, cuda)
        path = str(tmp_path / name)
        kept.append(sparse_loader(loader, N, net, cuda, 0.5, 128, 0, return_indices=True,
                                  subset_index_path=path, **kw)[2])
        metas.append(subset_index.read_subset_index(path)[1])
    assert kept[0] == kept[1] and metas[0] == metas[1]
    assert metas[0]["score_methods"] == ["el2n"] and metas[0]["select_by"] == "el2n"
    assert metas[0]["K"] == 1 and len(kept[0]) == _capi.keep_count(N, 0.5)
