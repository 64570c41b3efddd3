"""dd_nn_same_class on the device against the float64 restatement and the two bounds of
tests/test_nn_scores.py (the pick bound and the value bound, derived there), on that file's
inputs: class sizes that straddle the 32- and 128-wide tiles, a class of two, D = 512, a D that is
no multiple of 16, D = 1 and 17, an empty class, a class of one; duplicates, ties, non-finite
rows; and bitwise invariance over the batching, the order and the alignment of the queries.
"""
import numpy as np
import pytest
import torch

from data_diet_distributed_amd import _capi
from test_nn_scores import (CASES, TINY, class_order, d2_64, gap_floor, make_set, pick_bound,
                            ref_nn, value_bound)

pytestmark = pytest.mark.gpu

OPERANDS = ("f16x3", "bf16x3")


def run_nn(dev, f, labels, C, operands="f16x3", rows=None, perm=None, shift=0, accum=None):
    """The kernel on the rows of f [n, D]: candidates = all rows in class order; queries = the
    rows `rows` (default all), optionally permuted within their classes (`perm`: a seed), the
    buffers optionally placed `shift` floats into a larger allocation.  Returns (dist, nn_id)
    per query in the order of `rows` (NumPy)."""
    n = len(f)
    rows = np.arange(n) if rows is None else np.asarray(rows)
    c_order, c_off = class_order(labels, C)
    sub = labels[rows]
    if perm is None:
        q_local = np.argsort(sub, kind="stable")
    else:  # another order within each class
        rng = np.random.default_rng(perm)
        q_local = np.lexsort((rng.random(len(rows)), sub))
    q_rows = rows[q_local].astype(np.int64)
    q_off = np.zeros(C + 1, np.int64)
    q_off[1:] = np.cumsum(np.bincount(sub, minlength=C)[:C])

    def place(a, dtype):
        a = np.ascontiguousarray(a)
        buf = torch.zeros(a.size + shift + 8, dtype=dtype, device=dev)
        view = buf[shift:shift + a.size].view(a.shape)
        view.copy_(torch.from_numpy(a))
        return view

    q = place(f[q_rows], torch.float32)
    c = place(f[c_order], torch.float32)
    dist = torch.full((len(rows),), -7.0, dtype=torch.float32, device=dev)
    nn_id = torch.full((len(rows),), -7, dtype=torch.int64, device=dev)
    _capi.nn_same_class(q, place(q_rows, torch.int64), torch.from_numpy(q_off).to(dev), c,
                        place(c_order, torch.int64), torch.from_numpy(c_off).to(dev),
                        operands=operands, dist=dist, nn_id=nn_id, accum=accum)
    torch.cuda.synchronize()
    inv = np.empty(len(rows), np.int64)
    inv[q_local] = np.arange(len(rows))
    return dist.cpu().numpy()[inv], nn_id.cpu().numpy()[inv]


@pytest.fixture(scope="module")
def sets():
    """name -> (f, labels, C, (ref dist, best, gap)): computed once, shared, left unchanged."""
    out = {}
    for name, (sizes, D) in {**CASES, **TINY}.items():
        f, labels = make_set(sizes, D)
        out[name] = (f, labels, len(sizes), ref_nn(f[None], labels, len(sizes)))
    return out


def check(name, f, labels, C, ref, dist, nn_id, operands):
    """Every pick is another row of the same class; both bounds; the reference's pick wherever
    the gap is above the floor.  Returns the largest pick excess / bound."""
    ref_dist, best, gap = ref
    n, D = f.shape
    has = best[0] >= 0
    assert np.array_equal(nn_id >= 0, has)
    assert np.all(np.isinf(dist[~has])) and np.all(dist[~has] > 0) and np.all(nn_id[~has] == -1)
    rows = np.flatnonzero(has)
    pick = nn_id[rows]
    assert np.all(pick != rows) and np.all((pick >= 0) & (pick < n))
    assert np.array_equal(labels[pick], labels[rows])
    excess = d2_64(f, rows, pick) - d2_64(f, rows, best[0][rows])
    pb = pick_bound(f, labels, operands)[rows]
    want = np.sqrt(d2_64(f, rows, pick))
    err, tol = np.abs(dist[rows].astype(np.float64) - want), value_bound(D) * want
    ratio_v = (err[tol > 0] / tol[tol > 0]).max() if np.any(tol > 0) else 0.0
    print(f"nn {name} {operands}: pick excess / bound = {(excess / pb).max():.3g} "
          f"(largest excess {excess.max():.3g}, {int((pick != best[0][rows]).sum())} of "
          f"{len(rows)} picks differ), value error / bound = {ratio_v:.3g}")
    assert np.all(excess <= pb)
    assert np.all(err <= tol)
    clear = gap[0][rows] > gap_floor(f, labels)[rows]
    assert np.array_equal(pick[clear], best[0][rows][clear])
    return clear.mean()


@pytest.mark.parametrize("operands", OPERANDS)
@pytest.mark.parametrize("name", list(CASES))
def test_against_the_restatement(cuda, sets, name, operands):
    f, labels, C, ref = sets[name]
    dist, nn_id = run_nn(cuda, f, labels, C, operands)
    clear = check(name, f, labels, C, ref, dist, nn_id, operands)
    print(f"nn {name}: rows with a gap above the floor: {100 * clear:.1f} %")
    assert clear >= 0.9  # the equality above cannot pass by leaving rows out


@pytest.mark.parametrize("operands", OPERANDS)
@pytest.mark.parametrize("name", list(TINY))
def test_tiny_widths(cuda, sets, name, operands):
    f, labels, C, ref = sets[name]
    dist, nn_id = run_nn(cuda, f, labels, C, operands)
    check(name, f, labels, C, ref, dist, nn_id, operands)


@pytest.mark.parametrize("operands", OPERANDS)
def test_empty_class_and_class_of_one(cuda, operands):
    sizes, D = (40, 0, 1, 131, 0), 24  # classes 1 and 4 are empty, class 2 has one member
    f, labels = make_set(sizes, D, seed=9)
    ref = ref_nn(f[None], labels, len(sizes))
    dist, nn_id = run_nn(cuda, f, labels, len(sizes), operands)
    check("empty+single", f, labels, len(sizes), ref, dist, nn_id, operands)
    lone = int(np.flatnonzero(labels == 2)[0])
    assert dist[lone] == np.inf and nn_id[lone] == -1


def test_duplicates_ties_and_non_finite_rows(cuda):
    f, labels = make_set((150, 90, 60), 512)
    C = 3
    cls0 = np.flatnonzero(labels == 0)
    a, b = int(cls0[10]), int(cls0[140])       # an exact duplicate pair, 128+ rows apart
    f[b] = f[a]
    t = [int(v) for v in np.flatnonzero(labels == 1)[[3, 40, 77]]]  # three identical rows
    f[t[1]] = f[t[0]]
    f[t[2]] = f[t[0]]
    cls2 = np.flatnonzero(labels == 2)
    nan_row, inf_row = int(cls2[5]), int(cls2[33])
    f[nan_row, 100] = np.nan
    f[inf_row, 7] = np.inf
    for operands in OPERANDS:
        dist, nn_id = run_nn(cuda, f, labels, C, operands)
        assert dist[a] == 0.0 and dist[b] == 0.0 and nn_id[a] == b and nn_id[b] == a
        assert [dist[i] for i in t] == [0.0, 0.0, 0.0]
        assert [int(nn_id[i]) for i in t] == [t[1], t[0], t[0]]  # the smallest OTHER id
        # a non-finite candidate is never picked; a non-finite query gives NaN and -1
        assert not np.isin(nn_id, [nan_row, inf_row]).any()
        assert np.isnan(dist[nan_row]) and np.isnan(dist[inf_row])
        assert nn_id[nan_row] == -1 and nn_id[inf_row] == -1
        ok = np.setdiff1d(cls2, [nan_row, inf_row])
        assert np.all(np.isfinite(dist[ok])) and np.all(nn_id[ok] >= 0)
        # the finite rows of that class: the restatement without the two rows
        keep = np.setdiff1d(np.arange(len(f)), [nan_row, inf_row])
        ref = ref_nn(f[keep][None], labels[keep], C)
        got = keep[ref[1][0]]
        clear = ref[2][0] > gap_floor(f[keep], labels[keep])
        assert np.array_equal(nn_id[keep][clear], got[clear])


def test_bitwise_invariance(cuda, sets):
    """dist and nn_id of a row depend on the row, its class's candidate set and D: not on the
    batching of the queries, on nq, on their order or on the buffers' alignment."""
    for name in ("d64", "d100"):
        f, labels, C, _ = sets[name]
        n = len(f)
        for operands in OPERANDS:
            one = run_nn(cuda, f, labels, C, operands)
            parts = [np.arange(0, n // 3), np.arange(n // 3, n), np.arange(5, n, 7)]
            for rows in parts:  # a "shard": some queries against all candidates
                d, i = run_nn(cuda, f, labels, C, operands, rows=rows)
                assert np.array_equal(d.view(np.uint32), one[0][rows].view(np.uint32))
                assert np.array_equal(i, one[1][rows])
            for kw in ({"perm": 3}, {"shift": 1}, {"shift": 3, "perm": 8}):
                d, i = run_nn(cuda, f, labels, C, operands, **kw)
                assert np.array_equal(d.view(np.uint32), one[0].view(np.uint32)), (name, kw)
                assert np.array_equal(i, one[1]), (name, kw)


@pytest.mark.parametrize("name", ("d512", "d100", "d17"))
def test_dist_is_the_proto_score_against_the_pick(cuda, sets, name):
    """The value of a distance has one definition (the row reducer of csrc/dd_feat.h):
    dd_proto_scores with the candidate rows as centroids and every row labelled with the position
    of its nn pick gives nn's dist bit for bit."""
    f, labels, C, _ = sets[name]
    c_order, _ = class_order(labels, C)
    pos = np.empty(len(f), np.int64)  # id -> position among the candidates
    pos[c_order] = np.arange(len(f))
    q, c = torch.from_numpy(f).to(cuda), torch.from_numpy(f[c_order]).to(cuda)
    for operands in OPERANDS:
        dist, nn_id = run_nn(cuda, f, labels, C, operands)
        assert np.all(nn_id >= 0)  # (no class of one in these sets: every row has a pick)
        score = torch.full((len(f),), -7.0, dtype=torch.float32, device=cuda)
        _capi.proto_scores(q, torch.from_numpy(pos[nn_id]).to(cuda), c, score=score)
        assert np.array_equal(score.cpu().numpy().view(np.uint32), dist.view(np.uint32))


def test_accum_accumulates_and_outputs_are_optional(cuda, sets):
    f, labels, C, _ = sets["d64"]
    dist, _ = run_nn(cuda, f, labels, C)
    order, off = class_order(labels, C)
    rows = torch.from_numpy(f[order]).to(cuda)
    ids, off_d = torch.from_numpy(order).to(cuda), torch.from_numpy(off).to(cuda)
    acc = torch.full((len(f),), 2.0, dtype=torch.float32, device=cuda)
    ws = None
    for _ in range(2):
        ws = _capi.nn_same_class(rows, ids, off_d, rows, ids, off_d, accum=acc, workspace=ws)
    want = (np.float32(2.0) + dist[order]) + dist[order]
    assert np.array_equal(acc.cpu().numpy(), want.astype(np.float32))
    only_id = torch.empty(len(f), dtype=torch.int64, device=cuda)
    _capi.nn_same_class(rows, ids, off_d, rows, ids, off_d, nn_id=only_id, workspace=ws)
    assert np.array_equal(only_id.cpu().numpy(), run_nn(cuda, f, labels, C)[1][order])
    with pytest.raises(ValueError, match="no output"):
        _capi.nn_same_class(rows, ids, off_d, rows, ids, off_d)
