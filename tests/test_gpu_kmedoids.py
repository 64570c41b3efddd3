"""dd_kmedoids_greedy on the device against the float64 restatement of
tests/test_kmedoids_select.py.

Exact cases.  On integer-valued rows the operand halves, the products, the norms and every matrix
entry are integers below 2^24, and with n_g max d2 < 2^24 so is every partial sum of a gain:
picks, gains and cur must EQUAL the restatement's.  Entries in [-3, 3]: d2 <= 36 D <= 18 432
at n_g <= 301; the n = 5000 case has D = 2 and entries in [-15, 15]: 5000 * 1800 < 2^24.

The bound B.  Every matrix entry, and every cur (a minimum of entries), is within
E = 2 (eps + 2 u) max ||f||^2 of float64: eps = E_OP[operands] + (D + 2) 2^-24 is the key's
(tests/test_nn_scores.py), u = 2^-24, and adding the point's norm rounds twice more.  A term
max(cur_i - M[j][i], 0) is then within 2 E, and the fp32 sum of n_g non-negative terms adds
(n_g + 1) u relative:  B = 2 n_g E + (n_g + 1) u max gain.  The kernel takes the largest fp32
gain, so in float64 the pick's gain is at least the largest minus 2 B, and the reported gain is
within B of the pick's.  The cases are chosen (on the restatement alone) so that 2 B is below
1 % of a step's largest gain on at least 90 % of the steps: the slack cannot pass the check.
"""
import functools

import numpy as np
import pytest
import torch

from data_diet_distributed_amd import _capi
from test_gpu_kcenter import (READ_FIRST, S, SIZES4, bits, layout, pick_seeds, run_kc,
                              same_bits)
from test_kcenter_select import sq_dists64
from test_kmedoids_select import gains64, ref_kmedoids
from test_nn_scores import E_OP

pytestmark = pytest.mark.gpu

U = 2.0 ** -24


@pytest.fixture(autouse=True)
def through_run_kc(monkeypatch):
    """run_kc (tests/test_gpu_kcenter.py) drives the kernel: the two wrappers share their
    arguments and the shape of their results (picked, gain, cur)."""
    monkeypatch.setattr(_capi, "kcenter_greedy", _capi.kmedoids_greedy)


# (n, D, sizes, quotas, seeds per group, the entries' bound)
INT_CASES = {
    "n300_d512_g1_seed1": (300, 512, (300,), (40,), (1,), 3),
    "n301_d500_g1_seedS": (301, 500, (301,), (40,), (S,), 3),
    "n301_d17_g4_full": (301, 17, SIZES4, (130, 1, 0, 30), (S + 1, 1, 0, 1), 3),
    "n301_d1_g4_quota0": (301, 1, SIZES4, (20, 0, 0, 170), (S, 0, 0, S + 1), 3),
    "n300_d17_g1_seedS1": (300, 17, (300,), (30,), (S + 1,), 3),
    "n301_d512_g4": (301, 512, SIZES4, (50, 1, 0, 60), (1, 1, 0, S + 1), 3),
    # one group of 5000: the automatic workgroup count (313) is past READ_FIRST; D = 2 gives
    # hundreds of exact duplicates and ties at every step
    "n5000_d2_g1": (5000, 2, (5000,), (S + 1 + 6,), (S + 1,), 15),
}


@functools.lru_cache(maxsize=None)
def int_case(name):
    """(f, ids, groups, seeds, the planted duplicate of a seed, the restatement's outputs)"""
    n, D, sizes, quotas, counts, bound = INT_CASES[name]
    rng = np.random.default_rng(sum(map(ord, name)))
    f = rng.integers(-bound, bound + 1, size=(n, D)).astype(np.float32)
    groups = layout(n, sizes, rng)
    ids = rng.permutation(5 * n)[:n].astype(np.int64)  # distinct, not the positions
    seeds = pick_seeds(groups, counts, rng)
    # planted exact duplicates in group 0: of a seed, and a triple among the other rows
    s0 = seeds[groups[seeds] == 0][0]
    others = [r for r in np.nonzero(groups == 0)[0] if r not in set(seeds.tolist())]
    f[others[0]] = f[s0]
    f[others[1]] = f[others[2]]
    f[others[3]] = f[others[2]]
    return f, ids, groups, seeds, others[0], ref_kmedoids(f, ids, groups, seeds, quotas)


INT_RUNS = [(name, op, 0) for name in INT_CASES for op in ("f16x3", "bf16x3")] + [
    ("n5000_d2_g1", "f16x3", b) for b in (READ_FIRST, _capi.KCENTER_MAX_BLOCKS)]


@pytest.mark.parametrize("name,operands,blocks", INT_RUNS,
                         ids=[f"{n}-{o}-b{b}" for n, o, b in INT_RUNS])
def test_integer_rows_equal_the_restatement(cuda, name, operands, blocks):
    n, D, sizes, quotas, counts, _ = INT_CASES[name]
    f, ids, groups, seeds, dup, want = int_case(name)
    got = run_kc(cuda, f, ids, groups, quotas, seeds, operands=operands, blocks=blocks)
    assert np.array_equal(got[0], want[0])
    assert np.array_equal(got[1].astype(np.float64), want[1])
    assert np.array_equal(got[2].astype(np.float64), want[2])
    picks = [q - c for q, c in zip(quotas, counts)]
    for g in range(len(sizes)):
        mine = got[0][:picks[g], g].tolist() + ids[seeds[groups[seeds] == g]].tolist()
        assert len(set(mine)) == quotas[g] and -1 not in mine  # no row twice, no seed again
        if quotas[g] == 0 and sizes[g]:
            assert np.all(np.isposinf(got[2][groups == g]))
        if quotas[g] == sizes[g] and sizes[g] > 1:
            assert np.all(got[2][groups == g] == -1) and got[1][picks[g] - 1, g] == 0.0
        if quotas[g] == sizes[g] and g == 0:
            # filled completely: a duplicate of a kept row gains 0 and comes after every row
            # that gains something
            at = got[0][:picks[g], g].tolist().index(ids[dup])
            assert got[1][at, g] == 0.0 and np.all(got[1][at:picks[g], g] == 0.0)


GAUSS_CASES = {  # (n, D, sizes, quotas, seeds per group, operands)
    "n300_d17_g1_f16": (300, 17, (300,), (13,), (1,), "f16x3"),
    "n301_d17_g4_f16": (301, 17, SIZES4, (S + 8, 1, 0, S + 9), (S, 1, 0, S + 1), "f16x3"),
    "n301_d1_g4_f16": (301, 1, SIZES4, (5, 0, 0, 6), (1, 0, 0, 1), "f16x3"),
    "n300_d17_g1_bf16": (300, 17, (300,), (3,), (1,), "bf16x3"),
    "n301_d17_g4_bf16": (301, 17, SIZES4, (2, 1, 0, 2), (1, 1, 0, 1), "bf16x3"),
}


@functools.lru_cache(maxsize=None)
def gauss_case(name):
    n, D, sizes, quotas, counts, operands = GAUSS_CASES[name]
    rng = np.random.default_rng(sum(map(ord, name)) + 1)
    f = (np.maximum(rng.standard_normal((n, D)), 0.0) + 0.5).astype(np.float32)
    groups = layout(n, sizes, rng)
    ids = rng.permutation(3 * n)[:n].astype(np.int64)
    return f, ids, groups, quotas, pick_seeds(groups, counts, rng), counts, operands


def step_bound(f, member, operands, top):
    """B of the docstring for a step of the group `member` whose largest float64 gain is top"""
    eps = E_OP[operands] + (f.shape[1] + 2) * U
    E = 2 * (eps + 2 * U) * (f[member].astype(np.float64) ** 2).sum(axis=1).max()
    return 2 * len(member) * E + (len(member) + 1) * U * top


def replay(f, ids, groups, seeds, picks, picked, operands):
    """Every step in float64 from the picks `picked` [steps, G] themselves.  Returns (the steps
    as (g, t, B, the largest gain, the pick's gain), the final cur [n])."""
    steps, final = [], np.full(len(f), np.inf)
    for g in range(picked.shape[1]):
        member = np.nonzero(groups == g)[0]
        is_seed = np.isin(member, seeds)
        if not is_seed.any():
            continue
        M = sq_dists64(f[member])
        cur = M[is_seed].min(axis=0)
        cur[is_seed] = -1.0
        for t in range(picks[g]):
            gj = gains64(M, cur)
            gj[cur < 0] = -np.inf
            c = int(np.nonzero(ids[member] == picked[t, g])[0][0])  # a member (else IndexError)
            assert cur[c] >= 0, (g, t, "picked twice")
            steps.append((g, t, step_bound(f, member, operands, gj.max()), gj.max(), gj[c]))
            cur = np.minimum(cur, M[c])
            cur[c] = -1.0
        final[member] = cur
    return steps, final


@pytest.mark.parametrize("name", list(GAUSS_CASES))
def test_gaussian_rows_are_greedy_within_the_bound(cuda, name):
    f, ids, groups, quotas, seeds, counts, operands = gauss_case(name)
    picks = [q - c for q, c in zip(quotas, counts)]
    # the case is sharp: on the restatement's own steps 2 B is below 1 % of the largest gain
    ref = ref_kmedoids(f, ids, groups, seeds, quotas)
    sharp = [2 * B <= 0.01 * top
             for _, _, B, top, _ in replay(f, ids, groups, seeds, picks, ref[0], operands)[0]]
    assert len(sharp) == sum(picks) and np.mean(sharp) >= 0.9, np.mean(sharp)
    picked, gain, cur = run_kc(cuda, f, ids, groups, quotas, seeds, operands=operands)
    steps, final = replay(f, ids, groups, seeds, picks, picked, operands)
    for g, t, B, top, mine in steps:
        print(f"kmedoids {name} g{g} t{t}: |gain - gain64| / B = {abs(gain[t, g] - mine) / B:.3g}")
        assert mine >= top - 2 * B, (g, t, mine, top, B)
        assert abs(gain[t, g] - mine) <= B, (g, t, gain[t, g], mine, B)
    for g in range(len(quotas)):
        assert np.all(picked[picks[g]:, g] == -1) and np.all(gain[picks[g]:, g] == -1)
    assert np.array_equal(cur == -1, final == -1) and (cur == -1).sum() == sum(quotas)
    assert np.array_equal(np.isposinf(cur), np.isposinf(final))
    open_ = np.isfinite(final) & (final >= 0)  # every cur is within E (B's first term / 2 n_g)
    E = max(step_bound(f, np.arange(len(f)), operands, 0.0) / (2 * len(f)), 0.0)
    assert np.all(np.abs(cur[open_] - final[open_]) <= E)


def test_bitwise_invariance(cuda):
    """No output bit depends on the order of the input rows, the workgroup count, the seed
    batch, the buffer's placement or the other groups: group g of the four-group call equals a
    one-group call on that group's rows alone."""
    rng = np.random.default_rng(9)
    n, D, quotas, counts = 301, 500, (60, 1, 0, 40), (S + 1, 1, 0, S)
    f = (np.maximum(rng.standard_normal((n, D)), 0.0) + 0.5).astype(np.float32)
    f[rng.permutation(n)[:40]] = f[:40]  # exact duplicates: ties among the candidates
    groups = layout(n, SIZES4, rng)
    ids = rng.permutation(3 * n)[:n].astype(np.int64)
    seeds = pick_seeds(groups, counts, rng)
    base = run_kc(cuda, f, ids, groups, quotas, seeds)
    assert same_bits(run_kc(cuda, f, ids, groups, quotas, seeds, perm=rng.permutation(n)), base)
    for knobs in ({"blocks": 1}, {"blocks": 3}, {"blocks": READ_FIRST - 1},
                  {"blocks": READ_FIRST}, {"blocks": _capi.KCENTER_MAX_BLOCKS},
                  {"seed_batch": 1}, {"seed_batch": 3}, {"seed_batch": 64, "blocks": 7}):
        assert same_bits(run_kc(cuda, f, ids, groups, quotas, seeds, **knobs), base), knobs
    for g in range(len(quotas)):
        member = np.nonzero(groups == g)[0]
        if not len(member):
            continue
        local = {int(r): j for j, r in enumerate(member)}
        sub_seeds = np.array([local[int(r)] for r in seeds if groups[r] == g], dtype=np.int64)
        alone = run_kc(cuda, f[member], ids[member], np.zeros(len(member), np.int64),
                       [quotas[g]], sub_seeds)
        p = quotas[g] - counts[g]
        assert np.array_equal(alone[0][:, 0], base[0][:p, g]), g
        assert np.array_equal(bits(alone[1][:, 0]), bits(base[1][:p, g])), g
        assert np.array_equal(bits(alone[2]), bits(base[2][member])), g
    # the rows where they lie (one group, ids = positions: no sorting copy) at every alignment
    one, pos = np.zeros(n, np.int64), np.arange(n, dtype=np.int64)
    plain = run_kc(cuda, f, pos, one, [70], seeds, plain=True)
    assert same_bits(run_kc(cuda, f, pos, one, [70], seeds), plain)  # through the sort
    for shift in (1, 2, 3):
        assert same_bits(run_kc(cuda, f, pos, one, [70], seeds, shift=shift, plain=True),
                         plain), shift


def test_bad_rows_and_arguments_are_rejected(cuda):
    rng = np.random.default_rng(2)
    f = rng.standard_normal((300, 17)).astype(np.float32)
    groups, ids = layout(300, (100, 200), rng), np.arange(300, dtype=np.int64)
    f[7, 3], f[150, 0] = np.nan, np.inf
    with pytest.raises(ValueError, match="2 feature row"):
        run_kc(cuda, f, ids, groups, [5, 5], pick_seeds(groups, (1, 1), rng))
    rows = torch.zeros((8, 3), dtype=torch.float32, device=cuda)
    one = torch.zeros(1, dtype=torch.int64, device=cuda)
    for args, kw, msg in (((one, [1], [2]), {"operands": "fp32"}, "operands"),
                          ((one, [1], [8]), {}, "cannot keep"),
                          ((one[:0], [0], [2]), {}, "no seed")):
        with pytest.raises(ValueError, match=msg):
            _capi.kmedoids_greedy(rows, None, None, [8], *args, **kw)
