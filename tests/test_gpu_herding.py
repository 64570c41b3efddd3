"""dd_herding_greedy on the device against the float64 restatement of
tests/test_herding_select.py.

Exact cases.  Integer rows in [-3, 3], every row beside its negation (and one zero row where n_g
is odd): the group mean is exactly 0, P_i = ||f_i||^2, every matrix entry is an integer
<= 36 D, and with (quota + 1) 36 D < 2^24 so are every A_i and (t + 1) P_i: picks and values must
EQUAL the restatement's.  The 16-row case has entries in [-2, 2] and a mean that is a multiple
of 1/16: P is a multiple of 1/256 and still exact.

The bound B of the Gaussian case.  A matrix entry is within E = 2 (eps + 2 u) max ||f||^2 of
float64: eps = E_OP[operands] + (D + 2) 2^-24 is the key's (tests/test_nn_scores.py; the bound
tests/test_gpu_kmedoids.py states), u = 2^-24.  A_i adds t entries in fp32: t E + t u max A.  mu
is one rounding of a quotient exact to 2^-25: dmu = u ||mu|| + sqrt(D) 2^-25; P_i rounds D
differences and D fmaf steps, (D + 3) u P, and moves by 2 sqrt(P) dmu + dmu^2 with mu; the
final fma rounds once more.  So a device value is within
    B = t E + t u max A + (t + 1) ((D + 3) u max P + 2 sqrt(max P) dmu + dmu^2)
        + u max(max A, (t + 1) max P)
of float64's, and the pick's float64 value is at least the largest minus 2 B.
"""
import itertools

import numpy as np
import pytest
import torch

from data_diet_distributed_amd import _capi
from test_gpu_kcenter import bits, layout, pick_seeds
from test_herding_select import herding_values, ref_herding
from test_nn_scores import E_OP

pytestmark = pytest.mark.gpu

U = 2.0 ** -24


def run(dev, f, ids, groups, quotas, seeds, **kw):
    """(picked, value) of _capi.herding_greedy as NumPy arrays; ref_herding's arguments."""
    G = len(quotas)
    sizes = np.bincount(groups, minlength=G).tolist()
    counts = np.bincount(groups[seeds], minlength=G).tolist()
    to = lambda v: torch.from_numpy(np.ascontiguousarray(v)).to(dev)  # noqa: E731
    picked, value, _, _ = _capi.herding_greedy(
        to(f), to(ids), to(groups), sizes, to(seeds), counts,
        [int(q) - c for q, c in zip(quotas, counts)], **kw)
    return picked.cpu().numpy(), value.cpu().numpy()


def paired_rows(n_g, D, rng, bound=3):
    """n_g integer rows with mean exactly 0: n_g // 2 rows and their negations (two planted
    duplicates among them: ties), a zero row where n_g is odd; shuffled."""
    h = rng.integers(-bound, bound + 1, size=(n_g // 2, D))
    if len(h) > 3:
        h[1], h[3] = h[0], h[2]
    rows = np.concatenate([h, -h, np.zeros((n_g % 2, D), dtype=h.dtype)])
    return rows[rng.permutation(n_g)].astype(np.float32)


# (the last case: past 4 096 rows a thread of the select kernel owns sixteen rows, not four)
@pytest.mark.parametrize("n_g,D,G,several", list(itertools.product(
    (2, 65, 258, 1025), (8, 20, 72), (1, 3), (False, True))) + [(4098, 8, 1, True)])
def test_paired_integer_rows_equal_the_restatement(cuda, n_g, D, G, several):
    rng = np.random.default_rng(n_g * 1000 + D * 10 + G + several)
    # the other groups: six rows with an empty quota, and 33 rows
    sizes, quotas = ((n_g, 6, 33), [0, 0, 9]) if G == 3 else ((n_g,), [0])
    quotas[0] = n_g if n_g == 2 else 40  # the smallest case takes every row
    assert (max(quotas) + 1) * 36 * D < 2 ** 24
    counts = [min(5 if several else 1, q) for q in quotas]
    groups = layout(sum(sizes), sizes, rng)
    f = np.zeros((sum(sizes), D), dtype=np.float32)
    for g, s in enumerate(sizes):
        f[groups == g] = paired_rows(s, D, rng)
    ids = rng.permutation(5 * len(f))[:len(f)].astype(np.int64)
    seeds = pick_seeds(groups, counts, rng)
    want = ref_herding(f, ids, groups, seeds, quotas)
    got = run(cuda, f, ids, groups, quotas, seeds, operands="bf16x3" if D == 20 else "f16x3")
    assert np.array_equal(got[0], want[0])
    assert np.array_equal(got[1].astype(np.float64), want[1])


def test_nonzero_dyadic_mean_equals_the_restatement(cuda):
    rng = np.random.default_rng(16)
    f = rng.integers(-2, 3, size=(16, 8)).astype(np.float32)
    assert np.any(f.sum(axis=0) % 16)
    ids, groups = rng.permutation(40)[:16].astype(np.int64), np.zeros(16, np.int64)
    want = ref_herding(f, ids, groups, [11], [16])
    got = run(cuda, f, ids, groups, [16], np.array([11]))
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1].astype(np.float64), want[1])
    assert sorted(got[0][:, 0].tolist() + [ids[11]]) == sorted(ids.tolist())  # no row twice


@pytest.mark.parametrize("operands", ["f16x3", "bf16x3"])
def test_gaussian_rows_are_greedy_within_the_bound(cuda, operands):
    rng = np.random.default_rng(7)
    n, D, quotas, counts = 600, 64, (40, 40), (3, 1)
    f = (np.maximum(rng.standard_normal((n, D)), 0.0) + 0.5).astype(np.float32)
    groups = layout(n, (300, 300), rng)
    ids = rng.permutation(3 * n)[:n].astype(np.int64)
    seeds = pick_seeds(groups, counts, rng)
    picked, value = run(cuda, f, ids, groups, quotas, seeds, operands=operands)
    worst = 0.0
    for g in range(2):
        member = np.nonzero(groups == g)[0]
        fm = f[member].astype(np.float64)
        E = 2 * (E_OP[operands] + (D + 4) * U) * (fm ** 2).sum(axis=1).max()
        P = ((fm - fm.mean(axis=0)) ** 2).sum(axis=1).max()
        dmu = U * np.linalg.norm(fm.mean(axis=0)) + np.sqrt(D) * U / 2
        kept = [int(np.nonzero(member == s)[0][0]) for s in seeds[groups[seeds] == g]]
        for t in range(quotas[g] - counts[g]):
            v = herding_values(fm, kept)
            k = len(kept)
            A = (v[np.isfinite(v)] + (k + 1) * P).max()  # (an upper bound of the largest A)
            B = (k * E + k * U * A + (k + 1) * ((D + 3) * U * P + 2 * np.sqrt(P) * dmu + dmu ** 2)
                 + U * max(A, (k + 1) * P))
            c = int(np.nonzero(ids[member] == picked[t, g])[0][0])  # a member (else IndexError)
            assert c not in kept and v[c] >= v.max() - 2 * B, (g, t, v[c], v.max(), B)
            assert abs(value[t, g] - v[c]) <= B, (g, t, value[t, g], v[c], B)
            worst = max(worst, (v.max() - v[c]) / B)
            kept.append(c)
        assert np.all(picked[quotas[g] - counts[g]:, g] == -1)
    print(f"herding {operands}: largest regret / B = {worst:.3g}")


def test_bitwise_invariance(cuda):
    """No output bit depends on the mean's workgroup count, the order of the rows in the call or
    the numbering of the groups."""
    rng = np.random.default_rng(9)
    sizes, quotas, counts = (130, 70, 101), (60, 0, 40), (4, 0, 1)
    n, D = sum(sizes), 72
    f = (np.maximum(rng.standard_normal((n, D)), 0.0) + 0.5).astype(np.float32)
    f[rng.permutation(n)[:40]] = f[:40]  # exact duplicates: ties among the candidates
    groups = layout(n, sizes, rng)
    ids = rng.permutation(3 * n)[:n].astype(np.int64)
    seeds = pick_seeds(groups, counts, rng)
    base = run(cuda, f, ids, groups, quotas, seeds)
    for blocks in (1, 7):
        got = run(cuda, f, ids, groups, quotas, seeds, blocks=blocks)
        assert np.array_equal(got[0], base[0]) and np.array_equal(bits(got[1]), bits(base[1]))
    perm, p = rng.permutation(n), np.array([2, 0, 1])  # group g of the call is group p[g]
    inv = np.empty(n, dtype=np.int64)
    inv[perm] = np.arange(n)
    got = run(cuda, f[perm], ids[perm], p[groups[perm]], [quotas[g] for g in np.argsort(p)],
              inv[seeds])
    assert np.array_equal(got[0][:, p], base[0])
    assert np.array_equal(bits(got[1])[:, p], bits(base[1]))
