"""dd_logit_scores on the GPU against the NumPy float64 restatement (tests/test_logit_scores.py):
parity on every row family, accumulation and the Welford pair, edge rows, bad labels, bitwise
row independence and subsets.
"""
import numpy as np
import pytest
import torch

from data_diet_distributed_amd import _capi
from test_logit_scores import ATOL, RTOL, STATS, ref_logit_stats, ref_variability

pytestmark = pytest.mark.gpu

# one shape per row family of the kernel: LDS-staged rows at 1 / 2 / 4 lanes per row, 64 lanes
# per row, one block per row
FAMILIES = [(300, 10), (200, 100), (130, 1000), (40, 3000)]
FAMILY_IDS = ["lds16", "lds32x4", "rows", "wide"]


def run(cuda, lg, lb, stats=STATS, var=False, k=1, counter=None, into=None):
    """One dd_logit_scores launch into zeroed accumulators (or `into`) -> {name: ndarray}."""
    B = lg.shape[0]
    acc = into if into is not None else {}
    for m in stats:
        acc.setdefault(m, torch.zeros(B, device=cuda))
    kw = {m: acc[m] for m in stats}
    if var:
        acc.setdefault("var_mean", torch.full((B,), float("nan"), device=cuda))
        acc.setdefault("var_m2", torch.full((B,), float("nan"), device=cuda))
        kw.update(var_mean=acc["var_mean"], var_m2=acc["var_m2"], k=k)
    _capi.logit_scores(lg, lb, bad_labels=counter, **kw)
    return {m: v.cpu().numpy() for m, v in acc.items()}


def make(cuda, B, C, scale, seed=0):
    rng = np.random.default_rng(B * 100003 + C * 17 + seed)
    logits = (rng.normal(size=(B, C)) * scale).astype(np.float32)
    labels = rng.integers(0, C, size=B)
    return logits, labels, torch.from_numpy(logits).to(cuda), torch.from_numpy(labels).to(cuda)


def check_parity(got, ref):
    for m in ("loss", "entropy", "wrong_mass"):
        err = np.abs(got[m] - ref[m]) / (ATOL + RTOL * np.abs(ref[m]))
        print(f"{m}: max error / bound = {err.max():.3g}")
        np.testing.assert_allclose(got[m], ref[m], rtol=RTOL, atol=ATOL, err_msg=m)
    # one fp32 subtraction and one comparison: exact
    assert np.array_equal(got["margin"], ref["margin"].astype(np.float32))
    assert np.array_equal(got["error"], ref["error"].astype(np.float32))


@pytest.mark.parametrize("scale", [0.01, 4, 30])
@pytest.mark.parametrize("B,C", [(1, 2), (3, 2), (64, 10), (257, 10), (77, 16), (65, 17),
                                 (77, 100), (65, 128), (33, 129), (40, 1000), (9, 2049),
                                 (5, 5000)])
def test_matches_restatement(cuda, B, C, scale):
    logits, labels, lg, lb = make(cuda, B, C, scale)
    check_parity(run(cuda, lg, lb), ref_logit_stats(logits, labels))


def test_accumulators_add(cuda):
    logits, labels, lg, lb = make(cuda, 130, 10, 4)
    acc = {}
    first = run(cuda, lg, lb, into=acc)
    check_parity(first, ref_logit_stats(logits, labels))
    second = run(cuda, lg, lb, into=acc)
    for m in STATS:
        assert np.array_equal(second[m], 2 * first[m]), m


@pytest.mark.parametrize("B,C", [(300, 10), (40, 1000)])
def test_welford_matches_numpy_std(cuda, B, C):
    K = 10
    acc, w = {}, []
    for k in range(1, K + 1):
        logits, labels, lg, lb = make(cuda, B, C, 4, seed=k)
        labels = np.arange(B) % C  # the same labels for every checkpoint
        lb = torch.from_numpy(labels).to(cuda)
        run(cuda, lg, lb, stats=("wrong_mass",), var=True, k=k, into=acc)
        w.append(ref_logit_stats(logits, labels)["wrong_mass"])
    out = torch.empty(B, device=cuda)
    _capi.variability_finalize(acc["var_m2"], K, out)
    ref = ref_variability(w)
    got = out.cpu().numpy()
    print(f"variability: max |diff| = {np.abs(got - ref).max():.3g}")
    np.testing.assert_allclose(got, ref, rtol=RTOL, atol=ATOL)
    np.testing.assert_allclose(acc["var_mean"].cpu().numpy(), np.mean(w, axis=0), rtol=RTOL,
                               atol=ATOL)
    np.testing.assert_allclose(acc["wrong_mass"].cpu().numpy() / K, np.mean(w, axis=0),
                               rtol=RTOL, atol=ATOL)


@pytest.mark.parametrize("delta", [0.0, 1e-6])
def test_welford_nearly_equal_checkpoints(cuda, delta):
    """K checkpoints whose logits differ by `delta` per step (or not at all): the variability
    is ~0 and never NaN (M2 is clamped at 0 before the square root)."""
    B, C, K = 257, 10, 7
    logits, labels, _, lb = make(cuda, B, C, 2)
    acc, w = {}, []
    for k in range(1, K + 1):
        z = logits.copy()
        z[:, 1] += np.float32(delta * k)
        run(cuda, torch.from_numpy(z).to(cuda), lb, stats=(), var=True, k=k, into=acc)
        w.append(ref_logit_stats(z, labels)["wrong_mass"])
    out = torch.empty(B, device=cuda)
    _capi.variability_finalize(acc["var_m2"], K, out)
    got = out.cpu().numpy()
    assert np.isfinite(got).all() and (got >= 0).all()
    np.testing.assert_allclose(got, ref_variability(w), rtol=RTOL, atol=ATOL)
    if delta == 0.0:
        assert (got == 0).all()


def test_variability_finalize_clamps_and_keeps_nan(cuda):
    m2 = torch.tensor([4.0, -1e-12, float("nan"), 0.0, 9.0], device=cuda)
    out = torch.empty(5, device=cuda)
    _capi.variability_finalize(m2, 4, out)
    got = out.cpu().numpy()
    assert got[[0, 1, 3, 4]].tolist() == [1.0, 0.0, 0.0, 1.5] and np.isnan(got[2])


def test_saturated_rows(cuda):
    # the rows of test_el2n_extreme_logits: one logit dominates by 1e4
    logits = np.zeros((4, 10), np.float32)
    logits[:, 3] = 1e4
    labels = np.array([3, 0, 3, 9])
    got = run(cuda, torch.from_numpy(logits).to(cuda), torch.from_numpy(labels).to(cuda))
    assert all(np.isfinite(v).all() for v in got.values())
    check_parity(got, ref_logit_stats(logits, labels))
    assert got["loss"].tolist() == [0.0, 1e4, 0.0, 1e4]
    assert got["wrong_mass"].tolist() == [0.0, 1.0, 0.0, 1.0]
    assert got["entropy"].tolist() == [0.0] * 4


@pytest.mark.parametrize("B,C", FAMILIES, ids=FAMILY_IDS)
@pytest.mark.parametrize("value", [float("nan"), float("inf")], ids=["nan", "inf"])
def test_nonfinite_logit_gives_nan_rows(cuda, B, C, value):
    """A NaN or +inf logit anywhere in a row (the label's column, the first, the last, another)
    makes every requested statistic of that row NaN, also margin and error, which a plain fmaxf
    would let through; the other rows are bitwise those of the clean run."""
    logits, labels, lg, lb = make(cuda, B, C, 4)
    clean = run(cuda, lg, lb, var=True)
    rows = np.array([0, 5, B // 2, B - 1])
    cols = [int(labels[0]), 0, C - 1, (int(labels[B - 1]) + 1) % C]
    dirty = logits.copy()
    dirty[rows, cols] = value
    got = run(cuda, torch.from_numpy(dirty).to(cuda), lb, var=True)
    ok = np.setdiff1d(np.arange(B), rows)
    for m, v in got.items():
        assert np.isnan(v[rows]).all(), m
        assert np.array_equal(v[ok], clean[m][ok]), m
    ref = ref_logit_stats(dirty, labels)
    assert all(np.isnan(v[rows]).all() for v in ref.values())


@pytest.mark.parametrize("C", [2, 10, 100, 1000, 3000])
def test_all_tie_rows(cuda, C):
    B = 67
    logits = np.full((B, C), 0.5, np.float32)
    labels = np.arange(B) % C
    got = run(cuda, torch.from_numpy(logits).to(cuda), torch.from_numpy(labels).to(cuda))
    assert (got["error"] == 1).all() and (got["margin"] == 0).all()
    check_parity(got, ref_logit_stats(logits, labels))
    np.testing.assert_allclose(got["loss"], np.log(C), rtol=RTOL)
    np.testing.assert_allclose(got["wrong_mass"], 1 - 1 / C, rtol=RTOL)


@pytest.mark.parametrize("B,C", FAMILIES, ids=FAMILY_IDS)
def test_counts_bad_labels(cuda, B, C):
    """dd_el2n's rule (test_el2n_counts_bad_labels): a label outside [0, C) is counted once and
    its row is NaN in every statistic and in the Welford pair; the other rows are bitwise those
    of a clean run."""
    logits, labels, lg, _ = make(cuda, B, C, 4)
    bad_rows = np.array([0, 7, B // 2, B - 1])
    bad_labels = labels.copy()
    bad_labels[bad_rows] = [-1, C, C + 5, -(2 ** 40)]
    out = {}
    for name, lab in (("good", labels), ("bad", bad_labels)):
        cnt = _capi.label_counter(cuda)
        out[name] = (run(cuda, lg, torch.from_numpy(lab).to(cuda), var=True, counter=cnt),
                     int(cnt.item()))
    assert out["good"][1] == 0 and out["bad"][1] == bad_rows.size
    ok = np.setdiff1d(np.arange(B), bad_rows)
    for m, v in out["bad"][0].items():
        assert np.isnan(v[bad_rows]).all(), m
        assert np.array_equal(v[ok], out["good"][0][m][ok]), m
    assert np.isfinite(np.concatenate(list(out["good"][0].values()))).all()
    # a later checkpoint keeps the bad rows NaN
    acc = {m: torch.from_numpy(v).to(cuda) for m, v in out["bad"][0].items()}
    nxt = run(cuda, lg, torch.from_numpy(bad_labels).to(cuda), var=True, k=2, into=acc)
    for m, v in nxt.items():
        assert np.isnan(v[bad_rows]).all() and np.isfinite(v[ok]).all(), m


@pytest.mark.parametrize("C", [10, 100, 1000, 5000])
def test_rows_are_independent_of_batch_position_and_alignment(cuda, C):
    """Row r alone (B = 1) equals row r inside B = 257, bitwise; so do the rows of a
    logits[1:] slice and of a buffer that starts one float past a 16-byte boundary (the scalar
    staging path of the narrow rows)."""
    B = 257
    logits, labels, lg, lb = make(cuda, B, C, 4)
    full = run(cuda, lg, lb, var=True)
    for r in (0, 100, 256):
        one = run(cuda, lg[r:r + 1], lb[r:r + 1], var=True)
        for m in full:
            assert np.array_equal(one[m], full[m][r:r + 1]), (m, r)
    tail = run(cuda, lg[1:], lb[1:], var=True)
    flat = torch.empty(B * C + 1, device=cuda)
    flat[1:].copy_(lg.flatten())
    shifted = flat[1:].view(B, C)
    assert shifted.data_ptr() % 16 == 4
    off = run(cuda, shifted, lb, var=True)
    for m in full:
        assert np.array_equal(tail[m], full[m][1:]), m
        assert np.array_equal(off[m], full[m]), m


@pytest.mark.parametrize("B,C", FAMILIES, ids=FAMILY_IDS)
def test_subsets_equal_the_full_request(cuda, B, C):
    logits, labels, lg, lb = make(cuda, B, C, 4)
    full = run(cuda, lg, lb, var=True)
    for m in STATS:
        assert np.array_equal(run(cuda, lg, lb, stats=(m,))[m], full[m]), m
    pair = run(cuda, lg, lb, stats=(), var=True)
    assert set(pair) == {"var_mean", "var_m2"}
    assert np.array_equal(pair["var_mean"], full["var_mean"])
    assert np.array_equal(pair["var_mean"], full["wrong_mass"])  # k = 1: mean = w
    assert (pair["var_m2"] == 0).all()
    two = run(cuda, lg, lb, stats=("margin", "entropy"))
    assert np.array_equal(two["margin"], full["margin"])
    assert np.array_equal(two["entropy"], full["entropy"])


def test_empty_and_wrapper_checks(cuda):
    lg = torch.empty(0, 10, device=cuda)
    lb = torch.empty(0, dtype=torch.int64, device=cuda)
    _capi.logit_scores(lg, lb, loss=torch.empty(0, device=cuda))
    _capi.variability_finalize(torch.empty(0, device=cuda), 3, torch.empty(0, device=cuda))
    lg = torch.zeros(4, 10, device=cuda)
    lb = torch.zeros(4, dtype=torch.int64, device=cuda)
    acc = torch.zeros(4, device=cuda)
    with pytest.raises(ValueError, match="no statistic"):
        _capi.logit_scores(lg, lb)
    with pytest.raises(TypeError):
        _capi.logit_scores(lg.double(), lb, loss=acc)
    with pytest.raises(TypeError):
        _capi.logit_scores(lg, lb.int(), loss=acc)
    with pytest.raises(ValueError):
        _capi.logit_scores(lg.cpu(), lb, loss=acc)
    with pytest.raises(ValueError):
        _capi.logit_scores(lg, lb, loss=torch.zeros(5, device=cuda))
    with pytest.raises(ValueError, match="together"):
        _capi.logit_scores(lg, lb, var_mean=acc)
    with pytest.raises(_capi.DDError, match="C >= 2"):
        _capi.logit_scores(torch.zeros(4, 1, device=cuda), lb, margin=acc)
