"""dd_d2_weights, dd_d2_propagate and dd_d2_select on the device against the NumPy restatement of
tests/test_d2_select.py.

Exact cases: integer scores in [-4, 4], weights from {0, 0.25, 0.5, 1}.  Only ROWS_FRAC rows send
fractional weights (the others 0 or 1), so a score stays a multiple of 4^-8 far inside fp32's 24
bits (the restatement asserts that every updated score is a float32): fp32 arithmetic is exact and
the kernel must EQUAL the float64 loop.  Random cases: float scores, some negative, and weights in
[0, 1): every product and sum is rounded on its own, so the kernel must equal the same loop in
np.float32 bit for bit.  The sizes straddle one block of 256 rows, several blocks (4099) and a
second entry of the level above (16 643 > 64 blocks).  Even rows take their neighbours from their
own block, odd rows from anywhere; about one slot in seven is -1.
"""
import functools

import numpy as np
import pytest
import torch

from data_diet_distributed_amd import _capi
from test_d2_select import ref_propagate, ref_select

pytestmark = pytest.mark.gpu

ROWS_FRAC = 8
# (n, k, G): G = 3 has one quota of 0, one equal to the class size and one in between
CASES = [(1, 1, 1), (63, 5, 1), (64, 16, 3), (65, 1, 3), (257, 5, 1), (257, 16, 3),
         (4099, 5, 3), (4099, 16, 1), (16643, 5, 3)]


@functools.lru_cache(maxsize=None)
def inputs(n, k, G, exact):
    rng = np.random.default_rng(1000 * n + 10 * k + G + exact)
    own = (np.arange(n) // 256 * 256)[:, None] + rng.integers(0, 256, (n, k))
    nbr = np.where((np.arange(n) % 2 == 0)[:, None], np.minimum(own, n - 1),
                   rng.integers(0, n, (n, k)))
    nbr[rng.random((n, k)) < 0.15] = -1
    if exact:
        x = rng.integers(-4, 5, n).astype(np.float32)
        w = rng.integers(0, 2, (n, k)).astype(np.float32)
        frac = rng.choice(n, min(n, ROWS_FRAC), replace=False)
        w[frac] = rng.choice([0.0, 0.25, 0.5, 1.0], (len(frac), k))
    else:
        x = rng.random(n, dtype=np.float32) - np.float32(0.25)
        w = rng.random((n, k), dtype=np.float32)
    group, quota = None, [(n + 1) // 2]
    if G == 3:
        group = rng.integers(0, G, n)
        sizes = np.bincount(group, minlength=G)
        quota = [0, int(sizes[1]), int(sizes[2]) // 2]
    if n > 10000:  # (the restatement scans all rows per pick)
        quota = [min(q, 200) for q in quota]
    return x, nbr, w, group, quota


def dev(a, cuda):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(cuda)


@pytest.mark.parametrize("exact", [True, False], ids=["exact", "random"])
@pytest.mark.parametrize("n,k,G", CASES)
def test_select(cuda, n, k, G, exact):
    x, nbr, w, group, quota = inputs(n, k, G, exact)
    dt, bits = (np.float64, np.uint64) if exact else (np.float32, np.uint32)
    picked, value, skipped = ref_select(x, nbr, w, group, quota, dt, exact=exact)
    assert n < 63 or skipped > 0  # messages to rows already retired are part of the case
    got, val, bad = _capi.d2_select(dev(x, cuda), dev(nbr, cuda), dev(w, cuda), quota,
                                    dev(group, cuda))
    assert bad.item() == 0 and np.array_equal(got.cpu().numpy(), picked)
    assert np.array_equal(val.cpu().numpy().astype(dt).view(bits), value.view(bits))
    if G == 3:  # the quotas are met exactly: the rows past a full quota were dropped
        assert np.bincount(group[picked], minlength=G).tolist() == quota


def test_select_at_the_limits(cuda):
    """2^21 rows, 16 384 groups: the largest tables the workgroup's LDS is asked for.  Five planted
    scores, two past row 2^20 (the top level's second half), one in the last row; nbr[i] = i + 1."""
    n, G = _capi.D2_MAX_ROWS, _capi.D2_MAX_GROUPS
    plant = {5: 3.0, (1 << 20) + 77: 7.0, (1 << 20) + 78: 6.5, n - 1: 6.0, 4242: 5.0}
    x = np.zeros(n, dtype=np.float32)
    x[list(plant)] = list(plant.values())
    nbr = ((np.arange(n) + 1) % n)[:, None]
    w = np.full((n, 1), 0.5, dtype=np.float32)
    group = np.arange(n) % G
    quota = np.zeros(G, dtype=np.int64)
    quota[[5, 77, 78, (n - 1) % G]] = 1  # row 4242's group has none: dropped
    want = ref_select(x, nbr, w, group, quota.tolist(), np.float32)
    # 6.5 - 0.5 * 7 = 3.0 ties with row 5, which is the lower index
    assert want[0].tolist() == [(1 << 20) + 77, n - 1, 5, (1 << 20) + 78]
    got, val, bad = _capi.d2_select(dev(x, cuda), dev(nbr, cuda), dev(w, cuda), quota.tolist(),
                                    dev(group, cuda))
    assert bad.item() == 0 and got.tolist() == want[0].tolist()
    assert val.tolist() == want[1].tolist() == [7.0, 6.0, 3.0, 3.0]


@pytest.mark.parametrize("what", ["equal", "nan", "label"])
def test_select_ties_and_what_it_cannot_rank(cuda, what):
    x, nbr, w, group, quota = inputs(257, 16, 3, False)
    x, group = x.copy(), group.copy()
    if what == "equal":  # all-equal scores (0: every message is 0 too) come out in index order
        got = _capi.d2_select(dev(0 * x, cuda), dev(nbr, cuda), dev(w, cuda), [200])[0]
        assert got.tolist() == list(range(200))
        return
    if what == "nan":
        x[100] = np.nan
    else:
        group[7] = 3
    args = (dev(x, cuda), dev(nbr, cuda), dev(w, cuda), quota, dev(group, cuda))
    assert _capi.d2_select(*args, check=False)[2].item() == 1
    with pytest.raises(ValueError, match="d2: 1 non-finite"):
        _capi.d2_select(*args)


@pytest.mark.parametrize("exact", [True, False], ids=["exact", "random"])
@pytest.mark.parametrize("n,k", [(1, 1), (65, 16), (257, 5), (4099, 16)])
def test_propagate(cuda, n, k, exact):
    x, nbr, w, _, _ = inputs(n, k, 1, exact)
    dt = np.float64 if exact else np.float32
    got, bad = _capi.d2_propagate(dev(x, cuda), dev(nbr, cuda), dev(w, cuda))
    assert bad.item() == 0
    assert np.array_equal(got.cpu().numpy().astype(dt), ref_propagate(x, nbr, w, dt))


def test_weights(cuda):
    """w against float64 exp(-coef d^2).  The argument a = (coef * d) * d carries three fp32
    roundings (coef itself and the two products) of 2^-24 relative each, a 2^-24 of relative error
    each after the exponential; expf is documented to 1 ulp (2^-23 relative, its own rounding
    included).  a <= 60 keeps w a normal float."""
    rng = np.random.default_rng(5)
    n, k = 300, 7
    dist = rng.random((n, k), dtype=np.float32) * np.float32(4.0)
    nbr = rng.integers(0, n, (n, k))
    nbr[rng.random((n, k)) < 0.2] = -1
    dist[0, :3] = [np.inf, np.nan, 0.0]
    off = (nbr < 0) | ~np.isfinite(dist)
    for coef in (0.0, 0.37, 3.7):
        got = _capi.d2_weights(dev(dist, cuda), dev(nbr, cuda), coef).cpu().numpy()
        assert got.dtype == np.float32 and not got[off].any()
        a = coef * dist[~off].astype(np.float64) ** 2
        assert a.max() <= 60 and (coef or (got[~off] == 1.0).all())
        tol = np.expm1(3 * a * 2.0 ** -24) * (1 + 2.0 ** -23) + 2.0 ** -23
        assert (np.abs(got[~off] - np.exp(-a)) <= tol * np.exp(-a)).all()
