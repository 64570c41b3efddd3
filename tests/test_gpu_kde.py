"""dd_kde on the device against the restatement and the bound of tests/test_kde_scores.py, on the
inputs of tests/test_nn_scores.py in one, two and three ragged candidate segments; planted special
rows; bitwise invariance over the queries' batching and order; planted label noise."""
import numpy as np
import pytest
import torch

from data_diet_distributed_amd import _capi
from test_kde_scores import kde_bound, ref_kde
from test_nn_scores import CASES, TINY, make_set

pytestmark = pytest.mark.gpu

OPERANDS = ("f16x3", "bf16x3")
TAU = 0.25


def run_kde(dev, f, labels, inv, operands="f16x3", seg_rows=0, rows=None, shift=0, post=True):
    """Candidates = all rows of f, queries = the rows `rows` (default all) under their own ids,
    the buffers `shift` elements into a larger allocation.  Returns (nll, post) per query."""
    rows = np.arange(len(f)) if rows is None else np.asarray(rows)

    def place(a, dtype):
        a = np.ascontiguousarray(a)
        buf = torch.zeros(a.size + shift + 8, dtype=dtype, device=dev)
        view = buf[shift:shift + a.size].view(a.shape)
        view.copy_(torch.from_numpy(a))
        return view

    out = {"nll": torch.full((len(rows),), -7.0, dtype=torch.float32, device=dev)}
    if post:
        out.update(post=torch.full_like(out["nll"], -7.0), q_label=place(labels[rows], torch.int64),
                   c_label=place(labels, torch.int64))
    _capi.kde(place(f[rows], torch.float32), place(rows.astype(np.int64), torch.int64),
              place(f, torch.float32), place(np.arange(len(f)), torch.int64), inv,
              seg_rows=seg_rows, operands=operands, **out)
    torch.cuda.synchronize()
    return out["nll"].cpu().numpy(), out["post"].cpu().numpy() if post else None


def check(got, ref, bound, what):
    """nll within the bound, post within twice it; +inf exactly where the reference has it."""
    for name, g, r, b in (("nll", got[0], ref[0], bound), ("post", got[1], ref[1], 2 * bound)):
        fin = np.isfinite(r)
        err = np.abs(g[fin] - r[fin])
        print(f"kde {what} {name}: worst error {err.max():.3g}, error / bound <= "
              f"{(err / b[fin]).max():.3g}, bound >= {b.min():.3g}")
        assert np.array_equal(g[~fin], r[~fin]) and np.all(err <= b[fin]), (what, name)


@pytest.fixture(scope="module")
def sets():
    """name -> (f, labels, ref_kde): computed once, shared, left unchanged."""
    out = {}
    for name, (sizes, D) in {**CASES, **TINY}.items():
        f, labels = make_set(sizes, D)
        out[name] = (f, labels, ref_kde(f, labels, TAU))
    return out


@pytest.mark.parametrize("seg_rows", (0, 128, 256))
@pytest.mark.parametrize("operands", OPERANDS)
@pytest.mark.parametrize("name", list(CASES) + list(TINY))
def test_against_the_restatement(cuda, sets, name, operands, seg_rows):
    f, labels, ref = sets[name]
    got = run_kde(cuda, f, labels, ref[2], operands, seg_rows)
    check(got, ref, kde_bound(f, ref[2]), f"{name} {operands} seg_rows={seg_rows}")


@pytest.mark.parametrize("operands", OPERANDS)
def test_duplicates_an_outlier_non_finite_rows_and_a_class_of_one(cuda, sets, operands):
    f, labels, ref = sets["d512"]
    f, labels, inv = f.copy(), labels.copy(), ref[2]
    a, b, far, nan_row, lone = 10, 290, 77, 57, 201  # (a, b): in different candidate segments
    f[b] = f[a]
    f[far] += 100.0          # every t of this row is below -1000: a fixed reference gives +inf
    f[nan_row, 100] = np.nan
    labels[lone] = 99
    keep = np.setdiff1d(np.arange(len(f)), [nan_row])
    want = ref_kde(f[keep], labels[keep], None, inv=inv)
    assert -want[0][keep == far][0] * np.log2(np.e) < -1000 and np.isposinf(want[1][keep == lone])
    for seg_rows in (0, 128):
        nll, post = run_kde(cuda, f, labels, inv, operands, seg_rows)
        # a NaN row: NaN as a query, ignored as a candidate
        assert np.isnan(nll[nan_row]) and np.isnan(post[nan_row])
        check((nll[keep], post[keep]), want, kde_bound(f[keep], inv), f"planted {operands}")
        assert np.isfinite(nll[far]) and np.isposinf(post[lone])
    # an exact duplicate contributes weight exactly 1: alone with its twin, ln 1 = 0 both times
    for D in (512, 100, 17):
        two = np.repeat(sets["d512"][0][3:4, :D], 2, axis=0)
        nll, post = run_kde(cuda, two, np.zeros(2, np.int64), inv, operands)
        assert nll.tolist() == [0.0, 0.0] and post.tolist() == [0.0, 0.0]


def test_bitwise_invariance(cuda, sets):
    """No bit depends on the batching of the queries, nq, the rows' order, the buffers' alignment
    or whether the labels are passed."""
    for name in ("d64", "d100"):
        f, labels, ref = sets[name]
        n, inv = len(f), ref[2]
        perm = np.random.default_rng(4).permutation(n)
        for operands in OPERANDS:
            for seg_rows in (0, 128):
                one = run_kde(cuda, f, labels, inv, operands, seg_rows)
                for rows, kw in ((perm, {}), (np.arange(n // 3, n // 3 + 130), {}),
                                 (np.arange(5, n, 7), {"shift": 3}), (np.arange(n), {"shift": 1})):
                    got = run_kde(cuda, f, labels, inv, operands, seg_rows, rows=rows, **kw)
                    for g, o in zip(got, one):
                        assert np.array_equal(g.view(np.uint32), o[rows].view(np.uint32)), name
                two = [run_kde(cuda, f, labels, inv, operands, seg_rows, rows=r)
                       for r in (np.arange(0, 129), np.arange(129, n))]
                for i in (0, 1):
                    both = np.concatenate([two[0][i], two[1][i]])
                    assert np.array_equal(both.view(np.uint32), one[i].view(np.uint32)), name
                alone = run_kde(cuda, f, labels, inv, operands, seg_rows, post=False)[0]
                assert np.array_equal(alone.view(np.uint32), one[0].view(np.uint32))


def test_label_noise_is_what_kde_post_finds(cuda):
    """The planted set of tests/test_gpu_knn.py: four well-separated clusters, one per class, five
    rows carrying a wrong label.  Exactly those five are the top 5 by kde_post."""
    rng = np.random.default_rng(12)
    n, D = 260, 64
    labels = np.repeat(np.arange(4), n // 4).astype(np.int64)
    rng.shuffle(labels)
    centres = 10.0 * rng.standard_normal((4, D))
    noise = 0.1 * rng.standard_normal((n, D))
    flipped = np.array([3, 71, 128, 200, 255])
    noise[flipped] *= 3.0
    f = (centres[labels] + noise).astype(np.float32)
    noisy = labels.copy()
    noisy[flipped] = (labels[flipped] + np.array([1, 2, 3, 1, 2])) % 4
    ref = ref_kde(f, noisy, TAU)
    got = run_kde(cuda, f, noisy, ref[2])
    check(got, ref, kde_bound(f, ref[2]), "planted noise")
    top = _capi.select_topk(torch.from_numpy(got[1]).to(cuda), 5)[0]
    assert sorted(top.cpu().tolist()) == flipped.tolist()
