"""dd_cover_greedy on the device against the float64 restatement of tests/test_cover_select.py.

Every case is exact.  The rows are integers in [-3, 3] ([-1, 1] at D = 64) scaled by 1/8, every row beside its negation
(and one zero row where n_g is odd): a group's mean is exactly 0, P_i = ||f_i||^2 and every matrix
entry are multiples of 1/64 below 2^24 / 64, so M, P and their float64 sum are exact and theta is
the float of the reference's float64 value (1 ulp is allowed).  cover_radius is set per case so
that no matrix entry lies within 1e-3 (relative) of theta, which every case asserts on the
reference: the one compare cannot fall the other way, and from there on the rule is integers, so
picks, gains and `covered` must EQUAL the restatement's.
"""
import numpy as np
import pytest
import torch

from data_diet_distributed_amd import _capi
from test_cover_select import ref_cover
from test_gpu_kcenter import layout, pick_seeds

pytestmark = pytest.mark.gpu


def paired_rows(n_g, D, rng):
    b = 3 if D < 32 else 1  # (theta grows with D b^2 and the entries stay 1/64 apart)
    h = rng.integers(-b, b + 1, size=(n_g // 2, D))
    rows = np.concatenate([h, -h, np.zeros((n_g % 2, D), dtype=h.dtype)])
    return (rows[rng.permutation(n_g)] / 8.0).astype(np.float32)


def make(sizes, D, counts, rng):
    """(f, ids, groups, seeds, prio): paired rows per group, shuffled ids, counts[g] seeds and a
    prio that is a random permutation inside every group."""
    n = sum(sizes)
    groups = layout(n, sizes, rng)
    f, prio = np.zeros((n, D), dtype=np.float32), np.zeros(n, dtype=np.int32)
    for g, s in enumerate(sizes):
        f[groups == g], prio[groups == g] = paired_rows(s, D, rng), rng.permutation(s)
    ids = rng.permutation(5 * n)[:n].astype(np.int64)
    return f, ids, groups, pick_seeds(groups, counts, rng), prio


def run(dev, f, ids, groups, seeds, quotas, prio, radius, **kw):
    """(picked, gain, theta, covered, stat) of _capi.cover_greedy as NumPy arrays."""
    G = len(quotas)
    sizes = np.bincount(groups, minlength=G).tolist()
    counts = np.bincount(groups[seeds], minlength=G).tolist()
    to = lambda v: torch.from_numpy(np.ascontiguousarray(v)).to(dev)  # noqa: E731
    picked, gain, (theta, covered), stat = _capi.cover_greedy(
        to(f), to(ids), to(groups), sizes, to(seeds), counts,
        [int(q) - c for q, c in zip(quotas, counts)], to(prio), radius, check=False, **kw)
    return tuple(t.cpu().numpy() for t in (picked, gain, theta, covered, stat))


def check(dev, f, ids, groups, seeds, quotas, prio, radius, **kw):
    """Run, and hold the outputs to the restatement; returns (device outputs, reference)."""
    want = ref_cover(f, ids, groups, seeds, quotas, prio, radius)
    assert want[4] > 1e-3, f"an entry within {want[4]:.2e} of theta: choose another cover_radius"
    got = run(dev, f, ids, groups, seeds, quotas, prio, radius, **kw)
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
    assert np.array_equal(got[3], want[3])
    assert np.all(np.abs(got[2] - want[2]) <= np.spacing(want[2].astype(np.float32)))
    return got, want


# n_g: the word boundaries of a bit row, and one, four and sixteen rows per thread of the select
# kernel (<= 1 024, <= 4 096, above); a radius above 1/2 so that the balls hold many rows (the
# first gains at 4 098 x 17 are 869, 762, 309).  Beside the n_g rows: an empty group, six rows that keep
# their one seed alone (a zero quota of picks) and 33 rows that pick without a seed.
RADII = {(1, 17): 0.55, (1, 64): 0.55, (2, 17): 0.56, (2, 64): 0.55, (63, 17): 0.56,
         (63, 64): 0.56, (64, 17): 0.56, (64, 64): 0.56, (65, 17): 0.55, (65, 64): 0.55,
         (129, 17): 0.57, (129, 64): 0.56, (1025, 17): 0.57, (1025, 64): 0.55, (4098, 17): 0.55,
         (4098, 64): 0.56}


@pytest.mark.parametrize("n_g,D", sorted(RADII))
def test_picks_equal_the_restatement(cuda, n_g, D):
    rng = np.random.default_rng(1000 * n_g + D)
    sizes, quotas = (n_g, 0, 6, 33), [min(n_g, 40), 0, 1, 9]
    counts = [3 if n_g > 3 else 0, 0, 1, 0]
    f, ids, groups, seeds, prio = make(sizes, D, counts, rng)
    got, _ = check(cuda, f, ids, groups, seeds, quotas, prio, RADII[n_g, D],
                   operands="bf16x3" if D == 17 else "f16x3")
    assert got[4].tolist() == [0, 0] and got[3][1] == 0 and np.all(got[0][:, 1:3] == -1)
    assert len(set(got[0][got[0] >= 0].tolist()) | set(ids[seeds].tolist())) == sum(quotas)


def test_the_two_extreme_radii_pick_by_prio(cuda):
    rng = np.random.default_rng(5)
    n_g = 130
    f, ids, groups, seeds, prio = make((n_g,), 17, [0], rng)
    by_prio = ids[np.argsort(prio)]
    small, _ = check(cuda, f, ids, groups, seeds, [40], prio, 1e-6)  # only the own bit is set
    assert np.array_equal(small[0][:, 0], by_prio[:40]) and np.all(small[1] == 1)
    assert small[3][0] == 40
    large, _ = check(cuda, f, ids, groups, seeds, [40], prio, 1e3)  # one ball holds every row
    assert np.array_equal(large[0][:, 0], by_prio[:40])
    assert large[1][:, 0].tolist() == [n_g] + [0] * 39 and large[3][0] == n_g


def test_invariance_and_a_nan_row(cuda):
    """No output depends on the mean's workgroup count, the order of the rows in the call or the
    numbering of the groups; a row with a NaN is counted and never picked."""
    rng = np.random.default_rng(9)
    sizes, quotas, counts = (131, 70, 101), [60, 0, 40], [4, 0, 1]
    f, ids, groups, seeds, prio = make(sizes, 17, counts, rng)
    zero = np.nonzero((groups == 0) & ~f.any(axis=1) & ~np.isin(np.arange(len(f)), seeds))[0][0]
    f[zero, 3] = np.nan  # (the zero row of the odd group: the mean of the others stays 0)
    base, _ = check(cuda, f, ids, groups, seeds, quotas, prio, 0.6)
    assert base[4].tolist() == [1, 0] and ids[zero] not in base[0]
    for blocks in (1, 7):
        got = run(cuda, f, ids, groups, seeds, quotas, prio, 0.6, blocks=blocks)
        assert all(np.array_equal(a, b) for a, b in zip(got, base))
    perm, p = rng.permutation(len(f)), np.array([2, 0, 1])  # group g of the call is group p[g]
    inv = np.empty(len(f), dtype=np.int64)
    inv[perm] = np.arange(len(f))
    got = run(cuda, f[perm], ids[perm], p[groups[perm]], inv[seeds],
              [quotas[g] for g in np.argsort(p)], prio[perm], 0.6)
    for a, b in zip(got[:2], base[:2]):
        assert np.array_equal(a[:, p], b)
    assert np.array_equal(got[2][p], base[2]) and np.array_equal(got[3][p], base[3])
