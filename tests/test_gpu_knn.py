"""dd_knn on the device against the float64 restatement and the bounds of tests/test_knn_scores.py,
on the inputs of tests/test_nn_scores.py searched across classes (300 and 301 rows straddle the
32- and 128-wide tiles; D = 512; a D that is no multiple of 16; D = 1 and 17; fewer than k other
rows); duplicates, ties, non-finite rows; bitwise invariance over the candidate splits and over
the batching, the order and the ids of the queries; the accumulators; and what the scores mean
on planted label noise.
"""
import numpy as np
import pytest
import torch

from data_diet_distributed_amd import _capi
from test_gpu_nn import run_nn
from test_knn_scores import KS, check_picks, gap_floor, ref_knn
from test_nn_scores import CASES, TINY, make_set, value_bound

pytestmark = pytest.mark.gpu

OPERANDS = ("f16x3", "bf16x3")
OUTPUTS = ("dist", "nbr_id", "mean_dist", "disagree")


def run_knn(dev, f, labels, k, operands="f16x3", splits=0, rows=None, c_perm=None, shift=0):
    """The kernel on the rows of f [n, D], example r = row r: candidates = all rows (in the
    order `c_perm`, default ascending), queries = the rows `rows` (default all, in that order)
    under their own ids, the buffers optionally placed `shift` elements into a larger
    allocation.  Returns {output: NumPy array per query, in the order of `rows`}."""
    n = len(f)
    rows = np.arange(n) if rows is None else np.asarray(rows)
    cand = np.arange(n) if c_perm is None else np.asarray(c_perm)

    def place(a, dtype):
        a = np.ascontiguousarray(a)
        buf = torch.zeros(a.size + shift + 8, dtype=dtype, device=dev)
        view = buf[shift:shift + a.size].view(a.shape)
        view.copy_(torch.from_numpy(a))
        return view

    nq = len(rows)
    out = {"dist": torch.full((nq, k), -7.0, dtype=torch.float32, device=dev),
           "nbr_id": torch.full((nq, k), -7, dtype=torch.int64, device=dev),
           "mean_dist": torch.full((nq,), -7.0, dtype=torch.float32, device=dev),
           "disagree": torch.full((nq,), -7.0, dtype=torch.float32, device=dev)}
    _capi.knn(place(f[rows], torch.float32), place(rows.astype(np.int64), torch.int64),
              place(f[cand], torch.float32), place(cand.astype(np.int64), torch.int64), k,
              q_label=place(labels[rows], torch.int64), c_label=place(labels[cand], torch.int64),
              splits=splits, operands=operands, **out)
    torch.cuda.synchronize()
    return {name: t.cpu().numpy() for name, t in out.items()}


def same_bits(a, b):
    return all(np.array_equal(a[m].view(np.uint32) if a[m].dtype == np.float32 else a[m],
                              b[m].view(np.uint32) if b[m].dtype == np.float32 else b[m])
               for m in OUTPUTS)


@pytest.fixture(scope="module")
def sets():
    """name -> (f, labels, {k: ref_knn}): computed once, shared, left unchanged."""
    out = {}
    for name, (sizes, D) in {**CASES, **TINY}.items():
        f, labels = make_set(sizes, D)
        out[name] = (f, labels, {k: ref_knn(f[None], labels, k) for k in KS})
    return out


@pytest.mark.parametrize("operands", OPERANDS)
@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("name", list(CASES))
def test_against_the_restatement(cuda, sets, name, k, operands):
    f, labels, refs = sets[name]
    got = run_knn(cuda, f, labels, k, operands)
    clear = check_picks(f, labels, k, got["nbr_id"], got["dist"], got["mean_dist"],
                        got["disagree"], refs[k], operands, name)
    print(f"knn {name} k={k}: rows with a gap above the floor: {100 * clear:.1f} %")
    assert clear >= (0.55 if k == 16 else 0.80)  # the set equality cannot pass by leaving rows out


@pytest.mark.parametrize("operands", OPERANDS)
@pytest.mark.parametrize("name", list(TINY))
def test_tiny_widths_and_fewer_than_k_rows(cuda, sets, name, operands):
    f, labels, refs = sets[name]
    n = len(f)
    for k in KS[:2]:
        got = run_knn(cuda, f, labels, k, operands)
        check_picks(f, labels, k, got["nbr_id"], got["dist"], got["mean_dist"], got["disagree"],
                    refs[k], operands, name)
    # k = 16 > n - 1: every other row, then unused slots
    got = run_knn(cuda, f, labels, 16, operands, splits=3)
    assert n - 1 < 16
    for r in range(n):
        ids, d = got["nbr_id"][r], got["dist"][r]
        assert sorted(ids[:n - 1].tolist()) == [j for j in range(n) if j != r]
        assert np.all(np.isfinite(d[:n - 1]))
        want = np.sqrt(((f[r].astype(np.float64) - f[ids[:n - 1]]) ** 2).sum(axis=1))
        assert np.all(np.abs(d[:n - 1] - want) <= value_bound(f.shape[1]) * want)
        assert np.all(ids[n - 1:] == -1) and np.all(np.isposinf(d[n - 1:]))
    assert np.all(np.isposinf(got["mean_dist"])) and np.all(np.isnan(got["disagree"]))
    # ... and exactly k other rows is enough
    got = run_knn(cuda, f, labels, n - 1, operands)
    assert np.all(np.isfinite(got["mean_dist"])) and np.all(np.isfinite(got["disagree"]))
    assert np.all(got["nbr_id"] >= 0)


def test_duplicates_ties_and_non_finite_rows(cuda):
    f, labels = make_set((150, 90, 60), 512)
    k = 5
    a, b = 10, 290                       # an exact duplicate pair, in different candidate segments
    f[b] = f[a]
    t = [33, 140, 277]                   # three identical rows
    f[t[1]] = f[t[0]]
    f[t[2]] = f[t[0]]
    nan_row, inf_row = 57, 201
    f[nan_row, 100] = np.nan
    f[inf_row, 7] = np.inf
    keep = np.setdiff1d(np.arange(len(f)), [nan_row, inf_row])
    ref = ref_knn(f[keep][None], labels[keep], k)
    clear = ref[3][0] > gap_floor(f[keep])
    back = np.random.default_rng(2).permutation(len(f))
    for operands in OPERANDS:
        for kw in ({}, {"splits": 3}, {"splits": 7, "c_perm": back}):
            got = run_knn(cuda, f, labels, k, operands, **kw)
            dist, ids = got["dist"], got["nbr_id"]
            # an exact duplicate contributes exactly 0 and comes first
            assert dist[a][0] == 0.0 and dist[b][0] == 0.0 and ids[a][0] == b and ids[b][0] == a
            assert dist[a][1] > 0 and dist[b][1] > 0
            # three identical rows: the two others, the smaller id first
            for i, others in ((0, [t[1], t[2]]), (1, [t[0], t[2]]), (2, [t[0], t[1]])):
                assert ids[t[i]][:2].tolist() == others, (kw, i)
                assert dist[t[i]][:2].tolist() == [0.0, 0.0] and dist[t[i]][2] > 0
            # a non-finite candidate is never picked; a non-finite query gives NaN and -1
            assert not np.isin(ids, [nan_row, inf_row]).any()
            for r in (nan_row, inf_row):
                assert np.all(np.isnan(dist[r])) and np.all(ids[r] == -1)
                assert np.isnan(got["mean_dist"][r]) and np.isnan(got["disagree"][r])
            assert np.all(np.isfinite(got["mean_dist"][keep])) and np.all(ids[keep] >= 0)
            # the finite rows: the restatement without the two rows
            want = keep[ref[0][0]]
            assert np.array_equal(np.sort(ids[keep][clear], 1), np.sort(want[clear], 1))
            assert np.array_equal(got["disagree"][keep][clear],
                                  ref[2][clear].astype(np.float32))


def test_bitwise_invariance(cuda, sets):
    """Every output of a row depends on the row, the candidate set, D and k: not on the number of
    candidate segments (301 candidates in 3 or 7 segments: ragged, shorter than one 128-wide
    step), on the batching of the queries, on nq, on the rows' order or ids' offset, on the
    candidates' order or on the buffers' alignment."""
    for name in ("d64", "d100"):
        f, labels, _ = sets[name]
        n = len(f)
        rng = np.random.default_rng(4)
        for operands in OPERANDS:
            for k in (5, 16):
                one = run_knn(cuda, f, labels, k, operands, splits=1)
                for splits in (0, 2, 3, 7):
                    got = run_knn(cuda, f, labels, k, operands, splits=splits)
                    assert same_bits(got, one), (name, operands, k, splits)
                # a shard: a slice of the queries, under its rows' own ids, against everything
                lo, hi = n // 3, n // 3 + 130
                for rows, splits in ((np.arange(lo, hi), 0), (np.arange(lo, hi), 7),
                                     (np.arange(5, n, 7), 3)):
                    got = run_knn(cuda, f, labels, k, operands, splits=splits, rows=rows)
                    assert same_bits(got, {m: one[m][rows] for m in OUTPUTS}), (name, k, splits)
                perm = rng.permutation(n)
                got = run_knn(cuda, f, labels, k, operands, splits=2, rows=perm)
                assert same_bits(got, {m: one[m][perm] for m in OUTPUTS}), (name, k, "perm")
                two = [run_knn(cuda, f, labels, k, operands, splits=s, rows=r)
                       for r, s in ((np.arange(0, 129), 3), (np.arange(129, n), 0))]
                both = {m: np.concatenate([two[0][m], two[1][m]]) for m in OUTPUTS}
                assert same_bits(both, one), (name, k, "two batches")
                for kw in ({"c_perm": rng.permutation(n), "splits": 3}, {"shift": 1},
                           {"shift": 3, "splits": 7, "c_perm": rng.permutation(n)}):
                    got = run_knn(cuda, f, labels, k, operands, **kw)
                    assert same_bits(got, one), (name, operands, k, sorted(kw))


@pytest.mark.parametrize("name", ("d512", "d100", "d17"))
def test_k1_is_nn_same_class_over_one_class(cuda, sets, name):
    """The key of a pair and the value of a distance have one definition (csrc/dd_feat.h): with
    every row in one class, dd_nn_same_class's dist and nn_id are dd_knn(k = 1)'s first column
    bit for bit, whatever the split count; on three identical rows (exactly 0, the smallest other
    id) and on a row with a NaN (NaN and -1 as a query, never picked) too."""
    f = sets[name][0].copy()
    n, D = f.shape
    t = (1, n // 2, n - 2)
    f[t[1]] = f[t[0]]
    f[t[2]] = f[t[0]]
    nan_row = n // 3
    f[nan_row, D // 2] = np.nan
    one_class = np.zeros(n, np.int64)
    for operands in OPERANDS:
        dist, nn_id = run_nn(cuda, f, one_class, 1, operands)
        assert [dist[i] for i in t] == [0.0, 0.0, 0.0]
        assert [int(nn_id[i]) for i in t] == [t[1], t[0], t[0]]
        assert np.isnan(dist[nan_row]) and nn_id[nan_row] == -1
        assert not np.any(nn_id == nan_row)
        for splits in (1, 3):
            got = run_knn(cuda, f, one_class, 1, operands, splits=splits)
            assert np.array_equal(got["dist"][:, 0].view(np.uint32), dist.view(np.uint32))
            assert np.array_equal(got["nbr_id"][:, 0], nn_id)


def test_accumulators_accumulate_and_outputs_are_optional(cuda, sets):
    f, labels, _ = sets["d64"]
    n, k = len(f), 5
    one = run_knn(cuda, f, labels, k)
    x = torch.from_numpy(f).to(cuda)
    ids = torch.arange(n, dtype=torch.int64, device=cuda)
    lab = torch.from_numpy(labels).to(cuda)
    acc_d = torch.full((n,), 2.0, dtype=torch.float32, device=cuda)
    acc_s = torch.full((n,), 1.0, dtype=torch.float32, device=cuda)
    ws = None
    for _ in range(2):
        ws = _capi.knn(x, ids, x, ids, k, q_label=lab, c_label=lab, accum_dist=acc_d,
                       accum_disagree=acc_s, workspace=ws)
    assert ws.numel() == _capi.knn_workspace_bytes(n, n, f.shape[1], k)
    want = (np.float32(2.0) + one["mean_dist"]) + one["mean_dist"]
    assert np.array_equal(acc_d.cpu().numpy(), want.astype(np.float32))
    want = (np.float32(1.0) + one["disagree"]) + one["disagree"]
    assert np.array_equal(acc_s.cpu().numpy(), want.astype(np.float32))
    # every output alone; without labels where none is needed
    for name in OUTPUTS + ("accum_dist",):
        shape, dtype = ((n, k) if name in ("dist", "nbr_id") else (n,),
                        torch.int64 if name == "nbr_id" else torch.float32)
        t = torch.zeros(shape, dtype=dtype, device=cuda)
        kw = {"q_label": lab, "c_label": lab} if name == "disagree" else {}
        _capi.knn(x, ids, x, ids, k, workspace=ws, **kw, **{name: t})
        assert np.array_equal(t.cpu().numpy(), one[name.replace("accum_dist", "mean_dist")])
    with pytest.raises(ValueError, match="no output"):
        _capi.knn(x, ids, x, ids, k)
    with pytest.raises(ValueError, match="q_label"):
        _capi.knn(x, ids, x, ids, k, disagree=torch.zeros(n, device=cuda))
    for bad in (0, 17):
        with pytest.raises(ValueError, match="k must be"):
            _capi.knn(x, ids, x, ids, bad, mean_dist=torch.zeros(n, device=cuda))
    # no query: nothing to do
    _capi.knn(x[:0], ids[:0], x, ids, k, mean_dist=torch.zeros(0, device=cuda))


def test_label_noise_is_what_knn_disagree_finds(cuda):
    """Four well-separated clusters, one per class; five rows sit at the edge of their cluster
    (so that they are in no other row's neighbourhood) and carry a wrong label.  With k = 5
    exactly those five have knn_disagree == 1, all others 0, and a top-5 selection by
    knn_disagree returns them; by knn (the mean distance) they are the five most isolated."""
    rng = np.random.default_rng(12)
    n, D, k = 260, 64, 5
    labels = np.repeat(np.arange(4), n // 4).astype(np.int64)
    rng.shuffle(labels)
    centres = 10.0 * rng.standard_normal((4, D))
    noise = 0.1 * rng.standard_normal((n, D))
    flipped = np.array([3, 71, 128, 200, 255])
    noise[flipped] *= 3.0
    f = (centres[labels] + noise).astype(np.float32)
    noisy = labels.copy()
    noisy[flipped] = (labels[flipped] + np.array([1, 2, 3, 1, 2])) % 4
    got = run_knn(cuda, f, noisy, k)
    want = np.zeros(n, np.float32)
    want[flipped] = 1.0
    assert np.array_equal(got["disagree"], want)
    assert np.array_equal(labels[got["nbr_id"]], np.repeat(labels[:, None], k, axis=1))
    top = _capi.select_topk(torch.from_numpy(got["disagree"]).to(cuda), 5)[0]
    assert sorted(top.cpu().tolist()) == flipped.tolist()
    top = _capi.select_topk(torch.from_numpy(got["mean_dist"]).to(cuda), 5)[0]
    assert sorted(top.cpu().tolist()) == flipped.tolist()
