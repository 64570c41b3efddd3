"""dd_kcenter_greedy on the device against the float64 restatement of tests/test_kcenter_select.py.

Shapes: n = 300 and 301 rows (one past a multiple of the four rows a workgroup takes per pass,
as the knn tests straddle their tiles); D = 1 and 17 (rows that are not 16-byte aligned, a
single ragged pass), 500 (a ragged second pass), 512 and, once, PROTO_MAX_D at n = 64; one
group, and four groups of sizes (130, 1, 0, 170); 1, S and S + 1 seeds in a group (S = 8, the
default seed batch).

The bound g.  A squared distance is an fp32 sum of D terms (a_d - b_d)^2 >= 0.  Each
difference is rounded once (relative error u = 2^-24), which the square doubles; the product
is rounded once more unless it is fused into the addition (an FMA only removes that rounding);
and a term goes through at most D - 1 additions of non-negative partial sums, each rounded
once, whatever the order of the additions.  So every term, and hence the sum of these
non-negative terms, is within (1 + u)^(D + 2) - 1 = (D + 2) 2^-24 (to first order; the orders
used stay far inside it) of its float64 value:

    g = (D + 2) 2^-24.

The minimum over centres keeps the bound, so the kernel's mind2 is within g of float64.  The
kernel takes the row whose fp32 mind2 is largest: for the pick p and any unkept row j,
(1 + g) m_p >= fp32(m_p) >= fp32(m_j) >= (1 - g) m_j, so in float64 the pick's min squared
distance is at least (1 - g) / (1 + g) times the largest.  On integer-valued rows with entries
in [-15, 15] every partial sum is an integer below D 30^2 <= 2^24 at D <= 4096, so fp32 is
exact and the outputs must EQUAL the restatement's.
"""
import numpy as np
import pytest
import torch

from data_diet_distributed_amd import _capi
from test_kcenter_select import check_greedy, ref_kcenter

pytestmark = pytest.mark.gpu

S = 8  # the default seed batch
SIZES4 = (130, 1, 0, 170)


def g_of(D):
    return (D + 2) * 2.0 ** -24


def layout(n, sizes, rng):
    """int64 groups [n] of the given sizes, shuffled."""
    groups = np.repeat(np.arange(len(sizes)), sizes).astype(np.int64)
    assert len(groups) == n
    rng.shuffle(groups)
    return groups


def pick_seeds(groups, counts, rng):
    """counts[g] member rows of every group, in a shuffled order."""
    out = []
    for g, m in enumerate(counts):
        member = np.nonzero(groups == g)[0]
        out.extend(rng.permutation(member)[:m].tolist())
    return rng.permutation(np.array(out, dtype=np.int64))


def run_kc(dev, f, ids, groups, quotas, seeds, shift=0, perm=None, plain=False, **knobs):
    """The kernel through _capi.kcenter_greedy on the rows of f (in the order `perm`, with their
    ids and groups), the row buffer placed `shift` elements into a larger allocation.  plain:
    pass ids = groups = None (one group, ids = positions: the rows reach the kernel where they
    lie).  Returns (picked, radius2, mind2 in the order of f) as NumPy arrays."""
    n = len(f)
    perm = np.arange(n) if perm is None else np.asarray(perm)
    inv = np.empty(n, dtype=np.int64)
    inv[perm] = np.arange(n)
    G = len(quotas)
    sizes = [int((groups == g).sum()) for g in range(G)]
    counts = [int((groups[seeds] == g).sum()) for g in range(G)]
    picks = [int(q) - c for q, c in zip(quotas, counts)]
    a = np.ascontiguousarray(f[perm])
    buf = torch.zeros(a.size + shift + 8, dtype=torch.float32, device=dev)
    rows = buf[shift:shift + a.size].view(a.shape)
    rows.copy_(torch.from_numpy(a))
    to = lambda v: torch.from_numpy(np.ascontiguousarray(v)).to(dev)  # noqa: E731
    picked, radius2, mind2, _ = _capi.kcenter_greedy(
        rows, None if plain else to(ids[perm]), None if plain else to(groups[perm]), sizes,
        to(inv[seeds]), counts, picks, **knobs)
    torch.cuda.synchronize()
    return picked.cpu().numpy(), radius2.cpu().numpy(), mind2.cpu().numpy()[inv]


def bits(a):
    return a.view(np.uint32) if a.dtype == np.float32 else a


def same_bits(a, b):
    return all(np.array_equal(bits(x), bits(y)) for x, y in zip(a, b))


def int_rows(n, D, rng):
    return rng.integers(-15, 16, size=(n, D)).astype(np.float32)


# (n, D, sizes, quotas, seeds per group)
INT_CASES = {
    "n300_d512_g1_seed1": (300, 512, (300,), (40,), (1,)),
    "n301_d512_g1_seedS": (301, 512, (301,), (40,), (S,)),
    "n300_d500_g1_seedS1": (300, 500, (300,), (40,), (S + 1,)),
    "n301_d17_g4_full": (301, 17, SIZES4, (130, 1, 0, 30), (S + 1, 1, 0, 1)),
    "n301_d1_g4_full": (301, 1, SIZES4, (130, 1, 0, 30), (S, 1, 0, 1)),
    "n301_d500_g4_quota0": (301, 500, SIZES4, (20, 0, 0, 25), (1, 0, 0, S + 1)),
    "n301_d512_g4": (301, 512, SIZES4, (50, 1, 0, 60), (S, 1, 0, S + 1)),
    "n64_dmax_g1": (64, _capi.PROTO_MAX_D, (64,), (20,), (S + 1,)),
    # n >= 4096 in one group: the automatic workgroup count (ceil(n / 16) = 313) is past
    # READ_FIRST, where a workgroup reads the slot before its atomic; D = 2 gives hundreds of
    # exact duplicates and ties at every step
    "n5000_d2_g1_auto": (5000, 2, (5000,), (70,), (S + 1,)),
    "n4100_d17_g4_auto": (4100, 17, (4096, 1, 0, 3), (60, 1, 0, 2), (1, 1, 0, 1)),
}
READ_FIRST = 256  # workgroups per group from which the publish step reads the slot first


# every case at the automatic workgroup count; the large ones and two small ones also at the
# first count that reads the slot first and at the largest
INT_RUNS = [(name, 0) for name in INT_CASES] + [
    (name, b) for name in ("n5000_d2_g1_auto", "n4100_d17_g4_auto", "n301_d512_g4",
                           "n301_d1_g4_full")
    for b in (READ_FIRST, _capi.KCENTER_MAX_BLOCKS)]


@pytest.mark.parametrize("name,blocks", INT_RUNS, ids=[f"{n}-b{b}" for n, b in INT_RUNS])
def test_integer_rows_equal_the_restatement(cuda, name, blocks):
    n, D, sizes, quotas, counts = INT_CASES[name]
    rng = np.random.default_rng(sum(map(ord, name)))
    f = int_rows(n, D, rng)
    groups = layout(n, sizes, rng)
    ids = rng.permutation(5 * n)[:n].astype(np.int64)  # distinct, not the positions
    seeds = pick_seeds(groups, counts, rng)
    g0 = np.nonzero(groups == 0)[0]
    # planted exact duplicates in group 0: of a seed, and a triple among the other rows
    s0 = seeds[groups[seeds] == 0][0]
    others = [r for r in g0 if r not in set(seeds.tolist())]
    f[others[0]] = f[s0]
    f[others[1]] = f[others[2]]
    f[others[3]] = f[others[2]]
    want = ref_kcenter(f, ids, groups, seeds, quotas)
    got = run_kc(cuda, f, ids, groups, quotas, seeds, blocks=blocks)
    assert np.array_equal(got[0], want[0])
    assert np.array_equal(got[1].astype(np.float64), want[1])
    assert np.array_equal(got[2].astype(np.float64), want[2])
    picks = [q - c for q, c in zip(quotas, counts)]
    for g in range(len(sizes)):
        mine = got[0][:picks[g], g].tolist() + ids[seeds[groups[seeds] == g]].tolist()
        assert len(set(mine)) == quotas[g] and -1 not in mine  # no row twice, no seed again
        if quotas[g] == 0 and sizes[g]:
            assert np.all(np.isposinf(got[2][groups == g]))
        if quotas[g] == sizes[g] and sizes[g] > 1:  # filled completely: the duplicates come last
            assert np.all(got[2][groups == g] == -1) and got[1][picks[g] - 1, g] == 0.0
            assert ids[others[0]] in got[0][:picks[g], g]


def test_symmetric_ties_go_to_the_smaller_id(cuda):
    """The 16 corners of a hypercube around a seed at the centre: every corner ties at each
    step's front, so the picks are decided by the ids alone; then a ring of 12 points."""
    rng = np.random.default_rng(5)
    corners = np.array([[(i >> b & 1) * 2 - 1 for b in range(4)] for i in range(16)])
    ring = np.array([[3, 0, 0, 0], [-3, 0, 0, 0], [0, 3, 0, 0], [0, -3, 0, 0], [0, 0, 3, 0],
                     [0, 0, -3, 0], [0, 0, 0, 3], [0, 0, 0, -3], [3, 3, 0, 0], [-3, -3, 0, 0],
                     [0, 0, 3, 3], [0, 0, -3, -3]])
    f = np.concatenate([np.zeros((1, 4)), corners, ring]).astype(np.float32)
    n = len(f)
    groups = np.zeros(n, dtype=np.int64)
    for trial in range(3):
        ids = rng.permutation(1000)[:n].astype(np.int64)
        want = ref_kcenter(f, ids, groups, [0], [n])
        got = run_kc(cuda, f, ids, groups, [n], np.array([0]), perm=rng.permutation(n))
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
        assert np.all(got[2] == -1)


GAUSS_CASES = {
    "n300_d512_g1_seed1": (300, 512, (300,), (60,), (1,)),
    "n301_d500_g4": (301, 500, SIZES4, (130, 1, 0, 40), (S + 1, 1, 0, S)),
    "n301_d17_g4": (301, 17, SIZES4, (40, 0, 0, 170), (1, 0, 0, S + 1)),
    "n300_d1_g1_seedS": (300, 1, (300,), (50,), (S,)),
    "n64_dmax_g1": (64, _capi.PROTO_MAX_D, (64,), (24,), (1,)),
}


def gauss_case(name):
    n, D, sizes, quotas, counts = GAUSS_CASES[name]
    rng = np.random.default_rng(sum(map(ord, name)) + 1)
    f = (np.maximum(rng.standard_normal((n, D)), 0.0) + 0.5).astype(np.float32)
    if D == 1:
        f = rng.standard_normal((n, D)).astype(np.float32)
    groups = layout(n, sizes, rng)
    ids = rng.permutation(3 * n)[:n].astype(np.int64)
    return f, ids, groups, quotas, pick_seeds(groups, counts, rng), counts


@pytest.mark.parametrize("name", list(GAUSS_CASES))
def test_gaussian_rows_are_greedy_within_the_bound(cuda, name):
    f, ids, groups, quotas, seeds, counts = gauss_case(name)
    D = f.shape[1]
    g = g_of(D)
    picked, radius2, mind2 = run_kc(cuda, f, ids, groups, quotas, seeds)
    picks = [q - c for q, c in zip(quotas, counts)]
    # every step of every group, against the kernel's own earlier centres, in float64
    at_pick, final = check_greedy(f, ids, groups, seeds, picks, picked,
                                  slack=1.0 - (1.0 - g) / (1.0 + g))
    live = at_pick >= 0
    assert live.sum() == sum(picks)
    rel = np.abs(radius2[live] - at_pick[live]) / np.maximum(at_pick[live], 1e-300)
    print(f"kcenter {name}: g = {g:.3g}; radius2 rel err max {rel.max():.3g}")
    assert np.all(np.abs(radius2[live] - at_pick[live]) <= g * at_pick[live])
    assert np.all(radius2[~live] == -1)
    assert np.array_equal(mind2 == -1, final == -1) and (final == -1).sum() == sum(quotas)
    assert np.array_equal(np.isposinf(mind2), np.isposinf(final))
    fin = np.isfinite(final) & (final >= 0)
    assert np.all(np.abs(mind2[fin] - final[fin]) <= g * final[fin])


def test_bitwise_invariance(cuda):
    """No output bit depends on the order of the input rows, the seed batch, the workgroup
    count, or the other groups: group g of the four-group call equals a one-group call on that
    group's rows alone."""
    f, ids, groups, quotas, seeds, counts = gauss_case("n301_d500_g4")
    rng = np.random.default_rng(9)
    base = run_kc(cuda, f, ids, groups, quotas, seeds)
    for trial in range(2):
        assert same_bits(run_kc(cuda, f, ids, groups, quotas, seeds,
                                perm=rng.permutation(len(f))), base), trial
    for knobs in ({"seed_batch": 1}, {"seed_batch": 3}, {"seed_batch": 64}, {"blocks": 1},
                  {"blocks": 3}, {"blocks": 64}, {"seed_batch": 2, "blocks": 7},
                  {"blocks": READ_FIRST - 1}, {"blocks": READ_FIRST}, {"blocks": 1024},
                  {"blocks": _capi.KCENTER_MAX_BLOCKS}):
        assert same_bits(run_kc(cuda, f, ids, groups, quotas, seeds, **knobs), base), knobs
    # one group of 5 000 rows: the automatic count (313 workgroups) reads the slot first,
    # 64 workgroups publish directly
    big = np.random.default_rng(4)
    fb = (np.maximum(big.standard_normal((5000, 17)), 0.0) + 0.5).astype(np.float32)
    fb[big.permutation(5000)[:600]] = fb[:600]  # exact duplicates: ties among the candidates
    idb, gb = big.permutation(5000).astype(np.int64), np.zeros(5000, np.int64)
    sb = big.permutation(5000)[:3].astype(np.int64)
    base_b = run_kc(cuda, fb, idb, gb, [80], sb)
    for blocks in (64, READ_FIRST - 1, READ_FIRST, 1024, _capi.KCENTER_MAX_BLOCKS):
        assert same_bits(run_kc(cuda, fb, idb, gb, [80], sb, blocks=blocks), base_b), blocks
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


@pytest.mark.parametrize("D", [512, 500, 17])
def test_placement_changes_no_bit(cuda, D):
    """The rows where they lie (one group, ids = positions: no sorting copy), `shift` elements
    into a larger buffer: 16-byte aligned rows, and rows at every other alignment."""
    rng = np.random.default_rng(D)
    n = 301
    f = (np.maximum(rng.standard_normal((n, D)), 0.0) + 0.5).astype(np.float32)
    groups, ids = np.zeros(n, np.int64), np.arange(n, dtype=np.int64)
    seeds = rng.permutation(n)[:S + 1].astype(np.int64)
    base = run_kc(cuda, f, ids, groups, [70], seeds, plain=True)
    assert same_bits(run_kc(cuda, f, ids, groups, [70], seeds), base)  # through the sort
    for shift in (1, 2, 3, 4, 7):
        assert same_bits(run_kc(cuda, f, ids, groups, [70], seeds, shift=shift, plain=True),
                         base), shift


def test_bad_rows_and_ids_are_rejected(cuda):
    rng = np.random.default_rng(2)
    n, D = 300, 17
    f = rng.standard_normal((n, D)).astype(np.float32)
    groups = layout(n, (100, 200), rng)
    ids = np.arange(n, dtype=np.int64)
    seeds = pick_seeds(groups, (1, 1), rng)
    bad = f.copy()
    bad[7, 3] = np.nan
    bad[150, 0] = np.inf
    bad[151, 16] = -np.inf
    with pytest.raises(ValueError, match="3 feature row"):
        run_kc(cuda, bad, ids, groups, [5, 5], seeds)
    far = ids.copy()
    far[11] = 2 ** 31
    far[12] = -1
    with pytest.raises(ValueError, match="2 example id"):
        run_kc(cuda, f, far, groups, [5, 5], seeds)
    ok = ids.copy()
    ok[11] = 2 ** 31 - 1
    assert run_kc(cuda, f, ok, groups, [5, 5], seeds)[0].shape == (4, 2)
    # host-side rejections, before any launch
    rows = torch.zeros((4, 3), dtype=torch.float32, device=cuda)
    one = torch.zeros(1, dtype=torch.int64, device=cuda)
    with pytest.raises(ValueError, match="cannot keep"):
        _capi.kcenter_greedy(rows, None, None, [4], one, [1], [4])
    with pytest.raises(ValueError, match="no seed"):
        _capi.kcenter_greedy(rows, None, None, [4], one[:0], [0], [2])
