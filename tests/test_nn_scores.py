"""The nearest-same-class-neighbour score ("nn") on the host: a float64 NumPy restatement of the
definition, the two bounds the GPU tests hold the kernel to (derived below from the number
formats, then checked here against a plain-fp32 NumPy emulation of the kernel's key on the GPU
tests' own inputs), the config surface, and the entry points' argument checks, which run before
any device work.

    nn_i = min over j != i with y_j == y_i of || f_i - f_j ||_2, then the mean over K checkpoints

The pick bound.  The kernel picks the candidate with the smallest
    key(q, c) = ||c||^2 - 2 q.c        (= d^2(q, c) - ||q||^2)
computed in finite precision.  With u = 2^-24 (fp32's unit roundoff), per key:
  * q.c on split halves: every product drops lo.lo and the halves' residuals, at most
    e_op |q_d c_d| with e_op = 2^-22 (fp16 halves) or 2^-16 (bf16 halves), and an fp32
    accumulation of D terms in any order adds at most D u sum |q_d c_d|.  Since
    sum |q_d c_d| <= ||q|| ||c|| <= (||q||^2 + ||c||^2) / 2, the term 2 q.c is off by at most
    (e_op + D u) (||q||^2 + ||c||^2);
  * ||c||^2 and the one rounding of the final fused multiply-add are charged "+ 2 u": the norm is
    a sum of non-negative terms reduced as a tree (64 lanes, then a butterfly), and the D u above
    is the worst case of a sequential sum, which the MFMA's 16-wide steps do not reach.
So |key' - key| <= eps (||q||^2 + ||c||^2) with eps = e_op + (D + 2) 2^-24, and since the pick
has the smallest key',
    d^2(pick) - d^2(best) = key(pick) - key(best) <= 2 eps (||q||^2 + max_j ||c_j||^2).
This is worst-case arithmetic, not a measurement.

The value bound.  The returned distance is computed in fp32 from the fp32 rows: D non-negative
terms (each a rounded difference, squared) summed in any order stay within (D + 4) 2^-24
relative; the square root halves that and rounds once: (D / 2 + 2) 2^-24 relative to the float64
distance to the row nn_id names.
"""
import ctypes

import numpy as np
import pytest

from data_diet_distributed_amd import _capi, score as score_mod
from data_diet_distributed_amd import scoring
from data_diet_distributed_amd.scoring import (FEATURE_METHODS, FORWARD_FAMILY, LOGIT_FAMILY,
                                               ScoreConfig, ScoringEngine, pass_of)

E_OP = {"f16x3": 2.0 ** -22, "bf16x3": 2.0 ** -16}


# ---- restatement -------------------------------------------------------------------------------
def ref_nn(features, labels, C):
    """The definition in float64 on feature sets [K, n, D]: (dist [n], the mean over K of the
    distance to the nearest other row of the same class, +inf for a class of one; best [K, n],
    that row's index (ties to the smaller index), -1 without one; gap [K, n], second-best minus
    best squared distance, +inf with fewer than two candidates)."""
    features = np.asarray(features)
    labels = np.asarray(labels)
    K, n, _ = features.shape
    dist = np.zeros(n, np.float64)
    best = np.full((K, n), -1, np.int64)
    gap = np.full((K, n), np.inf)
    for k in range(K):
        f = features[k].astype(np.float64)
        d = np.full(n, np.inf)
        for c in range(C):
            idx = np.flatnonzero(labels == c)
            if len(idx) < 2:
                continue
            x = f[idx]
            d2 = ((x[:, None, :] - x[None, :, :]) ** 2).sum(axis=2)
            np.fill_diagonal(d2, np.inf)
            j = d2.argmin(axis=1)  # the first minimum: the smaller index
            best[k, idx] = idx[j]
            d[idx] = np.sqrt(d2[np.arange(len(idx)), j])
            if len(idx) > 2:
                two = np.partition(d2, 1, axis=1)[:, :2]
                gap[k, idx] = two[:, 1] - two[:, 0]
        dist += d
    return dist / K, best, gap


def pick_bound(f, labels, operands):
    """float64 [n]: the most d^2(pick) may exceed d^2(best) by, per row of f [n, D]."""
    f = np.asarray(f, np.float64)
    labels = np.asarray(labels)
    D = f.shape[1]
    eps = E_OP[operands] + (D + 2) * 2.0 ** -24
    sq = (f * f).sum(axis=1)
    cmax = np.zeros(len(f))
    for c in np.unique(labels):
        m = labels == c
        cmax[m] = sq[m].max()
    return 2 * eps * (sq + cmax)


def value_bound(D):
    """The relative error of a returned distance against float64 on the same two rows."""
    return (D / 2 + 2) * 2.0 ** -24


def gap_floor(f, labels):
    """float64 [n]: where the float64 gap between best and second-best d^2 exceeds this, the
    pick must be the reference's: 2^-12 (||q||^2 + max ||c||^2)."""
    f = np.asarray(f, np.float64)
    labels = np.asarray(labels)
    sq = (f * f).sum(axis=1)
    cmax = np.zeros(len(f))
    for c in np.unique(labels):
        m = labels == c
        cmax[m] = sq[m].max()
    return 2.0 ** -12 * (sq + cmax)


def d2_64(f, i, j):
    f = np.asarray(f, np.float64)
    return ((f[i] - f[j]) ** 2).sum(axis=-1)


# ---- inputs shared with the GPU tests ----------------------------------------------------------
SEED = 5
# (class sizes, D): sizes that straddle the 32- and 128-wide tiles, a class of two; a wide D; a D
# that is no multiple of 16
CASES = {
    "d64": ((70, 33, 2, 130, 64, 2), 64),
    "d512": ((150, 90, 60), 512),
    "d100": ((97, 203), 100),
}
TINY = {"d1": ((5, 3), 1), "d17": ((4, 6, 2), 17)}


def make_set(sizes, D, seed=SEED):
    """(fp32 [n, D], int64 labels [n]): rows of max(N(0, 1), 0) + 0.5 (a common positive
    component, as pooled post-ReLU rows have), labels shuffled."""
    rng = np.random.default_rng(seed)
    n = int(sum(sizes))
    f = (np.maximum(rng.standard_normal((n, D)), 0.0) + 0.5).astype(np.float32)
    labels = np.repeat(np.arange(len(sizes)), sizes).astype(np.int64)
    rng.shuffle(labels)
    return f, labels


def class_order(labels, C):
    """(order, offsets): the rows stable-sorted by label and the int64 [C + 1] class offsets, as
    the engine feeds the kernel."""
    labels = np.asarray(labels)
    order = np.argsort(labels, kind="stable").astype(np.int64)
    off = np.zeros(C + 1, np.int64)
    off[1:] = np.cumsum(np.bincount(labels, minlength=C)[:C])
    return order, off


def emulate_fp32_pick(f, labels, C):
    """The kernel's search with the key in plain fp32 (no split): ||c||^2 and q.c accumulated in
    fp32, key = ||c||^2 - 2 q.c, ties to the smaller index.  Returns the picked index per row."""
    f = np.asarray(f, np.float32)
    n = len(f)
    pick = np.full(n, -1, np.int64)
    sq = (f * f).sum(axis=1, dtype=np.float32)
    for c in range(C):
        idx = np.flatnonzero(labels == c)
        if len(idx) < 2:
            continue
        x = f[idx]
        dot = (x @ x.T).astype(np.float32)
        key = (sq[idx][None, :] - np.float32(2) * dot).astype(np.float32)
        np.fill_diagonal(key, np.inf)
        pick[idx] = idx[key.argmin(axis=1)]
    return pick


@pytest.mark.parametrize("name", list(CASES) + list(TINY))
def test_bounds_hold_for_plain_fp32_numpy(name):
    """The GPU tests' bounds, met by a plain-fp32 key on their inputs: a bound that fp32 itself
    misses would be wrong, not the kernel.  On the three main sets the fp32 key picks the true
    neighbour on every row, and at least 90 % of the rows have a gap above the floor at which the
    GPU tests demand the reference's pick."""
    sizes, D = (CASES.get(name) or TINY[name])
    f, labels = make_set(sizes, D)
    C = len(sizes)
    _, best, gap = ref_nn(f[None], labels, C)
    pick = emulate_fp32_pick(f, labels, C)
    assert np.array_equal(pick >= 0, best[0] >= 0)
    has = pick >= 0
    rows = np.flatnonzero(has)
    excess = d2_64(f, rows, pick[rows]) - d2_64(f, rows, best[0][rows])
    for ops in ("f16x3", "bf16x3"):
        ratio = excess / pick_bound(f, labels, ops)[rows]
        print(f"{name} {ops}: fp32 pick excess / bound = {ratio.max():.3g}")
        assert ratio.max() <= 1
    d32 = f[rows] - f[pick[rows]]
    got = np.sqrt((d32 * d32).sum(axis=1, dtype=np.float32))
    want = np.sqrt(d2_64(f, rows, pick[rows]))
    err, tol = np.abs(got - want), value_bound(D) * want  # (D = 1 has exact duplicates: 0 <= 0)
    print(f"{name}: fp32 value error / bound = {(err[tol > 0] / tol[tol > 0]).max():.3g}")
    assert np.all(err <= tol)
    if name in CASES:
        assert np.array_equal(pick, best[0])
        frac = np.mean(gap[0][rows] > gap_floor(f, labels)[rows])
        print(f"{name}: rows with a gap above the floor: {100 * frac:.1f} %")
        assert frac >= 0.9


def test_reference_on_a_hand_case():
    f = np.array([[0.0, 0], [3, 4], [0, 1], [10, 10], [3, 4], [7, 7]], np.float32)
    labels = np.array([0, 0, 0, 1, 0, 2])
    dist, best, gap = ref_nn(f[None], labels, 4)
    assert dist.tolist() == [1.0, 0.0, 1.0, np.inf, 0.0, np.inf]
    assert best[0].tolist() == [2, 4, 0, -1, 1, -1]
    assert gap[0][0] == 25.0 - 1.0 and gap[0][3] == np.inf
    two = ref_nn(np.stack([f, 2 * f]), labels, 4)[0]
    assert two[0] == 1.5 and two[1] == 0.0


# ---- host surface ------------------------------------------------------------------------------
def test_method_families():
    assert scoring.NEIGHBOR_METHODS == ("nn",)
    assert FEATURE_METHODS == ("proto",) and FORWARD_FAMILY == LOGIT_FAMILY + FEATURE_METHODS
    assert scoring.FORWARD_SCORES == FORWARD_FAMILY + scoring.NEIGHBOR_METHODS
    assert pass_of("nn") == "el2n" and pass_of("proto") == "el2n" and pass_of("grand") == "grand"


def test_score_config_accepts_nn():
    assert ScoreConfig(methods=("nn",), select_by="nn").methods == ("nn",)
    for ms in (("el2n", "nn"), ("nn", "grand"), ("proto", "nn"),
               LOGIT_FAMILY + ("proto", "nn", "grand")):
        for by in ms:
            assert ScoreConfig(methods=ms, select_by=by).select_by == by
    ScoreConfig(methods=("el2n", "nn"), select_by="nn", select_policy="balanced", select_skip=3)
    ScoreConfig(methods=("el2n", "nn"), select_by="el2n", refine=True)
    with pytest.raises(ValueError, match="refine"):
        ScoreConfig(methods=("el2n", "nn"), select_by="nn", refine=True)
    with pytest.raises(ValueError, match="unknown score method"):
        ScoreConfig(methods=("neighbour",), select_by="neighbour")
    with pytest.raises(ValueError, match="select_by"):
        ScoreConfig(methods=("el2n",), select_by="nn")


def test_auto_refinement_leaves_nn_alone():
    shell = ScoringEngine.__new__(ScoringEngine)
    shell.cfg = ScoreConfig(methods=("el2n", "nn"), select_by="nn", el2n_operands="bf16x3")
    assert not shell._refines("nn") and shell._refines("el2n")
    assert shell._f16_forward("nn") is False
    shell.cfg = ScoreConfig(methods=("el2n", "nn"), select_by="nn")
    assert shell._f16_forward("nn") is True  # the family's forward: redone on bf16 halves


def test_engine_config_maps_the_keys():
    cfg = {"batch_size": 128, "score_methods": ["el2n", "nn"], "select_by": "nn"}
    ecfg = score_mod.engine_config(cfg)
    assert ecfg.methods == ("el2n", "nn") and ecfg.select_by == "nn"
    assert score_mod.engine_config({"batch_size": 64, "score_methods": "nn"}).select_by == "nn"


def test_singleton_class_is_named():
    scoring.check_no_singleton_class([0, 2, 5, 3])
    with pytest.raises(ValueError, match="class 2 .*one member"):
        scoring.check_no_singleton_class([4, 0, 1, 3])


def test_exports_and_abi():
    for name in ("dd_nn_workspace_bytes", "dd_nn_same_class"):
        assert name in _capi.EXPORTS and hasattr(_capi.lib(), name)
    assert _capi.lib().dd_abi_version() == 10  # purely additive
    for name in ("nn_workspace_bytes", "nn_same_class"):
        assert callable(getattr(_capi, name))


def test_workspace_bytes():
    wb = _capi.nn_workspace_bytes
    # the halves of every row (hi and lo, 2 bytes each, D padded to 16), a norm per candidate and
    # a pick per query, each region rounded up to 256 bytes
    assert wb(256, 512, 64) == 4 * (256 + 512) * 64 + 4 * 512 + 4 * 256
    assert wb(256, 512, 49) == wb(256, 512, 64) and wb(256, 512, 65) == wb(256, 512, 80)
    assert wb(0, 0, 8) == 0 and wb(1, 1, 1, "bf16x3") == 4 * 256 + 2 * 256
    L = _capi.lib()
    for bad in ((-1, 4, 8, 1), (4, -1, 8, 1), (1 << 31, 4, 8, 1), (4, 1 << 31, 8, 1),
                (4, 4, 0, 1), (4, 4, 4097, 1), (4, 4, 8, 2), (4, 4, 8, -1)):
        assert L.dd_nn_workspace_bytes(*bad) == 0, bad


def test_entry_point_validates_before_launching():
    """Bad arguments give DD_EINVAL and a message before any device work, and nq == 0 returns
    DD_OK without a launch (so this runs without a GPU)."""
    L = _capi.lib()
    P16 = ctypes.c_void_p(16)
    big = 1 << 30

    def call(nq=4, nc=4, C=10, D=8, operands=1, q=P16, dist=P16, nn_id=P16, accum=P16, ws=P16,
             ws_bytes=big, q_off=P16, c=P16):
        return L.dd_nn_same_class(q, P16, q_off, nq, c, P16, P16, nc, C, D, operands, dist,
                                  nn_id, accum, ws, ws_bytes, None)

    for kw, word in (({"D": 0}, b"<= D"), ({"D": 4097}, b"<= D"), ({"C": 0}, b"<= C"),
                     ({"C": (1 << 20) + 1}, b"<= C"), ({"nq": -1}, b"nq"),
                     ({"nq": 1 << 31}, b"nq"), ({"nc": 1 << 31}, b"nc"),
                     ({"operands": 2}, b"operands"), ({"operands": -1}, b"operands"),
                     ({"q": None}, b"null"), ({"q_off": None}, b"null"), ({"c": None}, b"null"),
                     ({"dist": None, "nn_id": None, "accum": None}, b"no output"),
                     ({"ws": None}, b"workspace"), ({"ws_bytes": 64}, b"workspace"),
                     ({"ws": ctypes.c_void_p(24)}, b"aligned")):
        assert call(**kw) == -1, kw
        err = L.dd_last_error()
        assert err.startswith(b"dd_nn_same_class") and word in err, (kw, err)
    # nothing to do: DD_OK, whatever the data pointers
    assert call(nq=0) == 0 and L.dd_last_error() == b""
    assert call(nq=0, q=None, ws=None, ws_bytes=0, dist=None, nn_id=None) == 0
    assert call(nq=0, dist=None, nn_id=None, accum=None) == -1  # still no output requested
