"""The k-nearest-neighbour scores ("knn", "knn_disagree") on the host: a float64 NumPy restatement
of the definition, the bounds the GPU tests hold dd_knn to (those of tests/test_nn_scores.py,
restated for k picks below, then checked here against a plain-fp32 NumPy emulation of the
kernel's key on the GPU tests' own inputs), the config surface, and the entry points' argument
checks, which run before any device work.

    N_k(i)         = the k rows j != i of the whole set, any class, smallest (d^2(i, j), j)
    knn_i          = mean over j in N_k(i) of || f_i - f_j ||_2
    knn_disagree_i = |{ j in N_k(i) : y_j != y_i }| / k        (both: then the mean over K)

The pick bound.  Every key is off by at most eps (||q||^2 + ||c||^2), eps = e_op + (D + 2) 2^-24
(test_nn_scores.py derives it).  A pick p that is not among the true k best displaced a true
member t, so key'(p) <= key'(t), and d^2(t) <= d^2(k-th best):
    d^2(p) - d^2(k-th best) <= 2 eps (||q||^2 + max_j ||c_j||^2),  the max over the WHOLE set.

The value bound.  Each returned distance is within (D / 2 + 2) 2^-24 relative of the float64
distance to the row nbr_id names (test_nn_scores.py; the derivation leaves half an ulp of slack:
D + 2 roundings before the square root, halved, plus the root's own).  The kernel sums the k fp32
distances in double and rounds the mean once, which that half ulp covers: the mean is held to the
same bound against the float64 mean over the same picks.

The gap floor.  Where the float64 gap d^2_(k+1) - d^2_(k) exceeds 2^-12 (||q||^2 + max ||c||^2),
far above 2 eps of either operand kind at these widths, no row outside the true set can displace
a member: the neighbour SET must be the reference's, and knn_disagree must be equal exactly.
"""
import ctypes

import numpy as np
import pytest

from data_diet_distributed_amd import _capi, forward_scores, methods as methods_mod
from data_diet_distributed_amd import score as score_mod
from data_diet_distributed_amd import scoring
from data_diet_distributed_amd.scoring import LOGIT_FAMILY, ScoreConfig, ScoringEngine, pass_of
from test_nn_scores import CASES, E_OP, TINY, make_set, value_bound

KS = (1, 5, 16)


# ---- restatement -------------------------------------------------------------------------------
def sq_dists(f):
    """float64 [n, n]: squared distances between the rows of f, from the differences."""
    f = np.asarray(f, np.float64)
    out = np.empty((len(f), len(f)))
    for r0 in range(0, len(f), 64):
        out[r0:r0 + 64] = ((f[r0:r0 + 64, None, :] - f[None, :, :]) ** 2).sum(axis=2)
    return out


def ref_knn(features, labels, k):
    """The definition in float64 on feature sets [K, n, D]: (nbrs [K, n, k], each row's k nearest
    other rows ascending by (d^2, index), -1 in every slot when n - 1 < k; mean [n], the mean
    over K of the mean distance, +inf when n - 1 < k; disagree [n], the mean over K of the share
    of neighbours with another label, NaN when n - 1 < k; gap [K, n], d^2 of the (k + 1)-th
    nearest minus that of the k-th, +inf with fewer than k + 1 other rows)."""
    features = np.asarray(features)
    labels = np.asarray(labels)
    K, n, _ = features.shape
    nbrs = np.full((K, n, k), -1, np.int64)
    mean, dis = np.zeros(n), np.zeros(n)
    gap = np.full((K, n), np.inf)
    for c in range(K):
        if n - 1 < k:
            mean += np.inf
            dis += np.nan
            continue
        d2 = sq_dists(features[c])
        np.fill_diagonal(d2, np.inf)
        order = np.argsort(d2, axis=1, kind="stable")  # ties: the smaller index first
        nbrs[c] = order[:, :k]
        picked = np.take_along_axis(d2, nbrs[c], axis=1)
        mean += np.sqrt(picked).mean(axis=1)
        dis += (labels[nbrs[c]] != labels[:, None]).mean(axis=1)
        if n - 1 > k:
            gap[c] = d2[np.arange(n), order[:, k]] - picked[:, k - 1]
    return nbrs, mean / K, dis / K, gap


def scale_of(f):
    """float64 [n]: ||q||^2 + max_j ||c_j||^2, the max over the whole set."""
    sq = (np.asarray(f, np.float64) ** 2).sum(axis=1)
    return sq + sq.max()


def pick_bound(f, operands):
    D = np.shape(f)[1]
    return 2 * (E_OP[operands] + (D + 2) * 2.0 ** -24) * scale_of(f)


def gap_floor(f):
    return 2.0 ** -12 * scale_of(f)


def check_picks(f, labels, k, nbr, dist, mean, share, ref, operands, what=""):
    """One checkpoint's outputs of a search among the rows of f (row r is example r) against
    `ref` = ref_knn(f[None], labels, k): nbr int64 [n, k], dist fp32 [n, k], mean / share fp32
    [n] (share may be None).  The pick bound on every pick, the value bound on every distance and
    on the mean, nbr consistent with dist, and above the gap floor the reference's set and the
    exact disagreement.  Returns the share of rows above the gap floor."""
    nbrs, ref_mean, ref_dis, gap = ref
    n, D = f.shape
    assert n - 1 >= k
    rows = np.arange(n)[:, None]
    assert np.all((nbr >= 0) & (nbr < n)) and np.all(nbr != rows)
    assert all(len(set(r)) == k for r in nbr.tolist())
    d2 = sq_dists(f)
    got = np.take_along_axis(d2, nbr, axis=1)
    kth = d2[np.arange(n), nbrs[0][:, k - 1]]
    excess = (got - kth[:, None]).max(axis=1)
    pb = pick_bound(f, operands)
    want = np.sqrt(got)
    err, tol = np.abs(dist.astype(np.float64) - want), value_bound(D) * want
    m_want = want.mean(axis=1)
    m_err, m_tol = np.abs(mean.astype(np.float64) - m_want), value_bound(D) * m_want
    pos = tol > 0
    print(f"knn {what} k={k} {operands}: pick excess / bound = {(excess / pb).max():.3g}, "
          f"{int((np.sort(nbr, 1) != np.sort(nbrs[0], 1)).any(axis=1).sum())} of {n} sets "
          f"differ, value error / bound = {(err[pos] / tol[pos]).max() if pos.any() else 0:.3g}, "
          f"mean error / bound = {(m_err[m_tol > 0] / m_tol[m_tol > 0]).max():.3g}")
    assert np.all(excess <= pb)
    assert np.all(err <= tol) and np.all(m_err <= m_tol)
    # the slots ascend by (key, id): by distance up to the key's error
    assert np.all(np.diff(got, axis=1) >= -pb[:, None])
    clear = gap[0] > gap_floor(f)
    assert np.array_equal(np.sort(nbr[clear], 1), np.sort(nbrs[0][clear], 1))
    if share is not None:
        assert np.array_equal(share[clear], ref_dis[clear].astype(np.float32))
        own = (labels[nbr] != labels[:, None]).sum(axis=1).astype(np.float32) / np.float32(k)
        assert np.array_equal(share, own)  # always consistent with the ids returned
    return clear.mean()


def emulate_fp32(f, k):
    """dd_knn with the key in plain fp32 (no split): key = ||c||^2 - 2 q.c, ties to the smaller
    index; the distances in fp32 from the fp32 rows, their mean summed in double and rounded
    once.  Returns (nbr [n, k], dist fp32 [n, k], mean fp32 [n])."""
    f = np.asarray(f, np.float32)
    sq = (f * f).sum(axis=1, dtype=np.float32)
    key = (sq[None, :] - np.float32(2) * (f @ f.T).astype(np.float32)).astype(np.float32)
    np.fill_diagonal(key, np.inf)
    nbr = np.argsort(key, axis=1, kind="stable")[:, :k]
    diff = f[:, None, :] - f[nbr]
    dist = np.sqrt((diff * diff).sum(axis=2, dtype=np.float32))
    return nbr, dist, (dist.astype(np.float64).sum(axis=1) / k).astype(np.float32)


@pytest.fixture(scope="module")
def sets():
    return {name: make_set(sizes, D) for name, (sizes, D) in {**CASES, **TINY}.items()}


# (the tiny sets have 8 and 12 rows: k = 16 leaves them fewer than k other rows, which the GPU
# test checks for the +inf / -1 / NaN outputs)
@pytest.mark.parametrize("name,k", [(n, k) for n in CASES for k in KS]
                         + [(n, k) for n in TINY for k in KS[:2]])
def test_bounds_hold_for_plain_fp32_numpy(sets, name, k):
    """The GPU tests' bounds, met on ALL rows by a plain-fp32 key on their inputs: a bound that
    fp32 itself misses would be wrong, not the kernel.  On the three main sets the fp32 key picks
    the float64 set on every row, and enough rows lie above the gap floor that the set equality
    of the GPU tests cannot pass by leaving most rows out."""
    f, labels = sets[name]
    ref = ref_knn(f[None], labels, k)
    nbr, dist, mean = emulate_fp32(f, k)
    for ops in ("f16x3", "bf16x3"):
        frac = check_picks(f, labels, k, nbr, dist, mean, None, ref, ops, f"fp32 {name}")
    if name in CASES:
        assert np.array_equal(np.sort(nbr, 1), np.sort(ref[0][0], 1))  # (the set: not its order)
        print(f"{name} k={k}: rows with a gap above the floor: {100 * frac:.1f} %")
        assert frac >= (0.55 if k == 16 else 0.80)


def test_reference_on_a_hand_case():
    f = np.array([[0.0, 0], [3, 4], [0, 1], [10, 10], [3, 4], [7, 7]], np.float32)
    labels = np.array([0, 0, 0, 1, 0, 2])
    nbrs, mean, dis, gap = ref_knn(f[None], labels, 2)
    # rows 1 and 4 are duplicates; rows 0 and 3 see them at one distance: the smaller index
    assert nbrs[0].tolist() == [[2, 1], [4, 2], [0, 1], [5, 1], [1, 2], [3, 1]]
    assert mean[0] == 3.0 and mean[1] == np.sqrt(18.0) / 2 and mean[4] == mean[1]
    assert dis.tolist() == [0.0, 0.0, 0.0, 1.0, 0.0, 1.0]
    assert gap[0][0] == 0.0 and gap[0][1] == 25.0 - 18.0
    one = ref_knn(f[None], labels, 1)
    assert one[0][0][:, 0].tolist() == [2, 4, 0, 5, 1, 3] and one[3][0][0] == 24.0
    assert one[1][1] == 0.0 and one[1][4] == 0.0  # an exact duplicate contributes exactly 0
    two = ref_knn(np.stack([f, 2 * f]), labels, 2)
    assert two[1][0] == 4.5 and two[2].tolist() == dis.tolist()
    five = ref_knn(f[None], labels, 5)
    assert np.all(np.isinf(five[3])) and np.all(np.isfinite(five[1]))
    none = ref_knn(f[None], labels, 6)  # k > n - 1
    assert np.all(none[0] == -1) and np.all(np.isposinf(none[1])) and np.all(np.isnan(none[2]))


# ---- host surface ------------------------------------------------------------------------------
def test_method_families():
    assert scoring.KNN_METHODS == ("knn", "knn_disagree") == methods_mod.KNN_METHODS
    assert scoring.NEIGHBOR_METHODS == ("nn",)
    assert scoring.FORWARD_SCORES == scoring.FORWARD_FAMILY + scoring.NEIGHBOR_METHODS
    for m in scoring.KNN_METHODS:
        assert methods_mod.known(m) and pass_of(m) == "el2n" and not methods_mod.refinable(m)
    assert pass_of("grand") == "grand" and not methods_mod.known("knn_agree")


def test_score_config_accepts_the_knn_methods():
    assert ScoreConfig().knn_k == 5
    for m in scoring.KNN_METHODS:
        assert ScoreConfig(methods=(m,), select_by=m).methods == (m,)
    for ms in (("el2n", "knn"), ("knn_disagree", "grand"), ("proto", "nn", "knn", "knn_disagree"),
               LOGIT_FAMILY + ("proto", "nn", "knn", "knn_disagree", "grand")):
        for by in ms:
            assert ScoreConfig(methods=ms, select_by=by).select_by == by
    ScoreConfig(methods=("el2n", "knn_disagree"), select_by="knn_disagree",
                select_policy="balanced", select_skip=3, knn_k=16)
    ScoreConfig(methods=("el2n", "knn"), select_by="el2n", refine=True)
    for m in scoring.KNN_METHODS:
        with pytest.raises(ValueError, match="refine"):
            ScoreConfig(methods=("el2n", m), select_by=m, refine=True)
    with pytest.raises(ValueError, match="select_by"):
        ScoreConfig(methods=("el2n",), select_by="knn")
    for bad in (0, 17, -1, 2.0, True, "5"):
        with pytest.raises(ValueError, match="knn_k"):
            ScoreConfig(methods=("knn",), select_by="knn", knn_k=bad)
    assert ScoreConfig(methods=("el2n",), knn_k=0).knn_k == 0  # checked only where it is used
    assert _capi.KNN_MAX_K == 16


def test_auto_refinement_and_fallback_cover_the_knn_methods():
    shell = ScoringEngine.__new__(ScoringEngine)
    shell.cfg = ScoreConfig(methods=("el2n", "knn"), select_by="knn", el2n_operands="bf16x3")
    assert not shell._refines("knn") and shell._refines("el2n")
    assert shell._f16_forward("knn") is False
    shell.cfg = ScoreConfig(methods=("el2n", "knn_disagree"), select_by="knn_disagree")
    assert shell._f16_forward("knn_disagree") is True  # the family's forward: redone on bf16


def test_engine_config_maps_the_keys():
    cfg = {"batch_size": 128, "score_methods": ["el2n", "knn", "knn_disagree"],
           "select_by": "knn_disagree", "knn_k": 7}
    ecfg = score_mod.engine_config(cfg)
    assert ecfg.methods == ("el2n", "knn", "knn_disagree") and ecfg.select_by == "knn_disagree"
    assert ecfg.knn_k == 7
    assert score_mod.engine_config({"batch_size": 64, "score_methods": "knn"}).knn_k == 5
    with pytest.raises(ValueError, match="knn_k"):
        score_mod.engine_config({"batch_size": 64, "score_methods": "knn", "knn_k": 17})
    from data_diet_distributed_amd.config import DEFAULTS
    assert DEFAULTS["knn_k"] == 5


def test_small_dataset_is_named():
    forward_scores.check_knn_size(6, 5)
    with pytest.raises(ValueError, match="knn_k=5"):
        forward_scores.check_knn_size(5, 5)


def test_sparse_loader_checks_the_score_and_k():
    from data_diet_distributed_amd.get_scores_and_prune import sparse_loader
    with pytest.raises(ValueError, match="knn_k"):
        sparse_loader(None, 10, None, "cuda", 0.5, 4, 0, score="knn_disagree", knn_k=0)
    with pytest.raises(ValueError, match="refine"):
        sparse_loader(None, 10, None, "cuda", 0.5, 4, 0, score="knn", refine=True)
    with pytest.raises(ValueError, match="score must be"):
        sparse_loader(None, 10, None, "cuda", 0.5, 4, 0, score="knn_agree")


def test_exports_and_abi():
    for name in ("dd_knn_workspace_bytes", "dd_knn"):
        assert name in _capi.EXPORTS and hasattr(_capi.lib(), name)
    assert _capi.lib().dd_abi_version() == 10  # purely additive
    for name in ("knn_workspace_bytes", "knn"):
        assert callable(getattr(_capi, name))


def test_workspace_bytes():
    wb = _capi.knn_workspace_bytes
    # the halves of every row (hi and lo, 2 bytes each, D padded to 16), a norm per candidate and
    # the partial lists (a key and a row number per query, segment and slot), each region rounded
    # up to 256 bytes
    assert wb(256, 512, 64, 5, 3) == 4 * (256 + 512) * 64 + 4 * 512 + 2 * (256 * 3 * 5 * 4)
    assert wb(256, 512, 49, 5, 3) == wb(256, 512, 64, 5, 3)
    assert wb(256, 512, 65, 5, 3) == wb(256, 512, 80, 5, 3)
    assert wb(1, 1, 1, 1, 1, "bf16x3") == 4 * 256 + 256 + 2 * 256 and wb(0, 0, 8, 1, 1) == 0
    # splits = 0: from nq and nc alone, two workgroups per compute unit (512 over the query
    # tiles) where a segment keeps four 128-candidate steps
    assert wb(256, 512, 64, 5, 0) == wb(256, 512, 64, 5, 1)      # 512 candidates: one segment
    assert wb(50000, 50000, 512, 5, 0) == wb(50000, 50000, 512, 5, 2)    # 391 tiles
    assert wb(6250, 50000, 512, 5, 0) == wb(6250, 50000, 512, 5, 11)     # 49 tiles: a shard of 8
    assert wb(128, 1 << 20, 64, 16, 0) == wb(128, 1 << 20, 64, 16, 64)   # never above 64
    assert wb(6250, 50000, 512, 5, 11) > wb(6250, 50000, 512, 5, 1)
    L = _capi.lib()
    for bad in ((-1, 4, 8, 5, 0, 1), (4, -1, 8, 5, 0, 1), (1 << 31, 4, 8, 5, 0, 1),
                (4, 1 << 31, 8, 5, 0, 1), (4, 4, 0, 5, 0, 1), (4, 4, 4097, 5, 0, 1),
                (4, 4, 8, 0, 0, 1), (4, 4, 8, 17, 0, 1), (4, 4, 8, 5, -1, 1), (4, 4, 8, 5, 65, 1),
                (4, 4, 8, 5, 0, 2), (4, 4, 8, 5, 0, -1)):
        assert L.dd_knn_workspace_bytes(*bad) == 0, bad


def test_entry_point_validates_before_launching():
    """Bad arguments give DD_EINVAL and a message before any device work, and nq == 0 returns
    DD_OK without a launch (so this runs without a GPU)."""
    L = _capi.lib()
    P16 = ctypes.c_void_p(16)
    big = 1 << 30
    outs = ("dist", "nbr_id", "mean_dist", "disagree", "accum_dist", "accum_disagree")

    def call(nq=4, nc=4, D=8, k=5, splits=0, operands=1, q=P16, q_id=P16, q_label=P16, c=P16,
             c_id=P16, c_label=P16, ws=P16, ws_bytes=big, **out):
        ptrs = [out.get(name, P16) for name in outs]
        return L.dd_knn(q, q_id, q_label, nq, c, c_id, c_label, nc, D, k, splits, operands, *ptrs,
                        ws, ws_bytes, None)

    none = {name: None for name in outs}
    for kw, word in (({"D": 0}, b"<= D"), ({"D": 4097}, b"<= D"), ({"k": 0}, b"<= k"),
                     ({"k": 17}, b"<= k"), ({"splits": -1}, b"splits"),
                     ({"splits": 65}, b"splits"), ({"nq": -1}, b"nq"), ({"nq": 1 << 31}, b"nq"),
                     ({"nc": 1 << 31}, b"nc"), ({"nc": -1}, b"nc"),
                     ({"operands": 2}, b"operands"), ({"operands": -1}, b"operands"),
                     ({"q": None}, b"null"), ({"q_id": None}, b"null"), ({"c": None}, b"null"),
                     ({"c_id": None}, b"null"), ({"q_label": None}, b"label"),
                     ({"c_label": None}, b"label"),
                     ({"q_label": None, "disagree": None}, b"label"),  # accum_disagree is asked
                     (none, b"no output"),
                     ({"ws": None}, b"workspace"), ({"ws_bytes": 64}, b"workspace"),
                     ({"ws": ctypes.c_void_p(24)}, b"aligned")):
        assert call(**kw) == -1, kw
        err = L.dd_last_error()
        assert err.startswith(b"dd_knn") and word in err, (kw, err)
    # the size of the workspace follows `splits` as passed
    need = _capi.knn_workspace_bytes(300, 300, 64, 5, 7)
    assert call(nq=300, nc=300, D=64, splits=7, ws_bytes=need - 1) == -1
    assert b"workspace" in L.dd_last_error()
    # nothing to do: DD_OK, whatever the data pointers
    assert call(nq=0) == 0 and L.dd_last_error() == b""
    assert call(nq=0, q=None, q_id=None, q_label=None, ws=None, ws_bytes=0, dist=None) == 0
    assert call(nq=0, **none) == -1  # still no output requested
    # the binding checks the same before it touches the library
    import torch
    x = torch.zeros((4, 8))
    with pytest.raises(ValueError, match="GPU tensor"):
        _capi.knn(x, None, x, None, 5, mean_dist=torch.zeros(4))
