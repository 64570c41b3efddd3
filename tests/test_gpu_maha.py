"""dd_maha_scatter and dd_maha_dist on the device against the float64 restatement and the bounds of
tests/test_maha_scores.py (derived there from the number formats).

Shapes: N = 300 and 301 rows (two segments of 256 rows, the second ragged; three 128-row tiles of
the distance kernel), classes of sizes (130, 1, 0, 170) or one class of all N; D = 1 and 17 (rows
not 16-byte aligned, a ragged K step), 128 and 129 (one output tile, and one column past it),
500 and 512 (four column slabs, the triangular skip over four output blocks).

Exact scatter: integer rows in +- pairs around an integer class offset make every class mean and
every a_i an integer with |a| <= 15, which one operand half holds exactly, and every partial sum
an integer below 301 * 15^2 < 2^24: S must EQUAL the restatement's.  No slack beyond the derived
bounds is used anywhere.
"""
import numpy as np
import pytest
import torch

from data_diet_distributed_amd import _capi, forward_scores
from test_gpu_kcenter import bits, layout, same_bits
from test_maha_scores import dist_bound, ref_maha, scatter_bound

pytestmark = pytest.mark.gpu

SIZES4 = (130, 1, 0, 170)
OPERANDS = ("f16x3", "bf16x3")


def to(dev, a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def device_inputs(dev, f, labels, C):
    """(rows, labels, counts, mean) on the device: the class means as proto forms them."""
    rows, lab = to(dev, f), to(dev, labels)
    counts, _ = _capi.class_counts(lab, C, check=True)
    mean, _ = forward_scores.class_means(rows, lab, counts)
    return rows, lab, counts, mean


def gaussian_rows(n, D, sizes, seed):
    """max(N(0, 1), 0) + 0.5 scaled per column by 1 .. 30: post-ReLU-like, anisotropic."""
    rng = np.random.default_rng(seed)
    f = np.maximum(rng.standard_normal((n, D)), 0) + 0.5
    return (f * np.linspace(1, 30, D)).astype(np.float32), layout(n, sizes, rng)


def paired_int_rows(n, D, sizes, rng):
    """Integer rows off_c +- v in pairs (an odd class also holds off_c itself), |v| <= 15."""
    labels = layout(n, sizes, rng)
    f = np.zeros((n, D), np.float32)
    for c, m in enumerate(sizes):
        idx = np.flatnonzero(labels == c)
        off = rng.integers(-8, 9, size=D)
        v = rng.integers(-15, 16, size=(m // 2, D))
        f[idx[:m // 2]], f[idx[m // 2:2 * (m // 2)]] = off + v, off - v
        f[idx[2 * (m // 2):]] = off
    return f, labels


@pytest.mark.parametrize("operands", OPERANDS)
@pytest.mark.parametrize("D", [1, 17, 128, 129, 500])
@pytest.mark.parametrize("n,sizes", [(301, SIZES4), (300, (300,)), (301, (301,))],
                         ids=["n301_c4", "n300_c1", "n301_c1"])
def test_scatter_is_exact_on_integer_rows(cuda, n, sizes, D, operands):
    f, labels = paired_int_rows(n, D, sizes, np.random.default_rng(D + n))
    assert _capi.maha_segment_rows(n, D) < n  # more than one segment
    S, bad, _ = _capi.maha_scatter(*device_inputs(cuda, f, labels, len(sizes)), operands=operands)
    assert int(bad.item()) == 0
    assert np.array_equal(S.cpu().numpy(), ref_maha(f, labels, len(sizes), 1.0)["S"])


@pytest.mark.parametrize("operands", OPERANDS)
@pytest.mark.parametrize("D,shrink", [(17, 0.0), (17, 0.01), (129, 0.0), (129, 1.0), (512, 0.01),
                                      (512, 1.0)])
def test_gaussian_rows_within_the_bounds(cuda, D, shrink, operands):
    n = 301
    f, labels = gaussian_rows(n, D, SIZES4, 7 + D)
    ref = ref_maha(f, labels, 4, shrink)
    bound = dist_bound(ref, operands)
    live = ref["maha"] > 0  # (all but the single-row class)
    assert live.sum() == 300
    assert np.mean(bound[live] < 0.01 * ref["maha"][live] ** 2) >= 0.9  # sharp on the reference

    rows, lab, counts, mean = device_inputs(cuda, f, labels, 4)
    S, _, ws = _capi.maha_scatter(rows, lab, counts, mean, operands=operands)
    sb = scatter_bound(ref, operands, _capi.maha_segment_rows(n, D))
    S = S.cpu().numpy()
    assert np.array_equal(S, S.T)
    r_s = np.max(np.abs(S - ref["S"]) / np.maximum(sb, 1e-300))
    dist = torch.empty(n, dtype=torch.float32, device=cuda)
    _capi.maha_dist(rows, lab, counts, mean, to(cuda, ref["W"].astype(np.float32)),
                    operands=operands, dist=dist, workspace=ws)
    got = dist.cpu().numpy().astype(np.float64)
    r_d = np.max(np.abs(got[live] ** 2 - ref["maha"][live] ** 2) / bound[live])
    print(f"D={D} shrink={shrink} {operands}: largest error / bound: S {r_s:.3f}, maha^2 {r_d:.3f}")
    assert r_s <= 1 and r_d <= 1 and got[~live] == 0


def test_dist_is_bitwise_independent_of_position_and_alignment(cuda):
    n, D = 301, 129
    f, labels = gaussian_rows(n, D, SIZES4, 3)
    rows, lab, counts, mean = device_inputs(cuda, f, labels, 4)
    W = to(cuda, ref_maha(f, labels, 4, 0.01)["W"].astype(np.float32))

    def run(r, y):
        out = torch.empty(r.shape[0], dtype=torch.float32, device=cuda)
        _capi.maha_dist(r, y, counts, mean, W, dist=out)
        return out.cpu().numpy()

    base = run(rows, lab)
    assert base[labels == 1] == 0 and np.isfinite(base).all()  # the single-row class: exactly 0
    perm = np.random.default_rng(5).permutation(n)
    assert same_bits([run(to(cuda, f[perm]), to(cuda, labels[perm]))], [base[perm]])
    for shift in (1, 2, 3):  # 4, 8 and 12 bytes
        buf = torch.zeros(n * D + 4, dtype=torch.float32, device=cuda)
        moved = buf[shift:shift + n * D].view(n, D).copy_(rows)
        assert same_bits([run(moved, lab)], [base])
    for i in (0, 200, 300):
        assert bits(run(rows[i:i + 1].clone(), lab[i:i + 1].clone()))[0] == bits(base)[i]


@pytest.mark.parametrize("value", [float("nan"), float("inf")])
def test_non_finite_rows_are_counted_and_rejected(cuda, value):
    f, labels = gaussian_rows(301, 17, SIZES4, 11)
    f[[5, 250], [3, 16]] = value
    with pytest.raises(ValueError, match=r"maha: 2 feature row\(s\).*\(2 non-finite\)"):
        forward_scores.maha(to(cuda, f), to(cuda, labels), 4)


def test_indefinite_covariance_names_the_shrinkage(cuda):
    f, labels = gaussian_rows(301, 512, SIZES4, 13)  # N - C < D: S is singular
    with pytest.raises(ValueError, match="maha_shrink"):
        forward_scores.maha(to(cuda, f), to(cuda, labels), 4, shrink=0.0)
    assert bool(torch.isfinite(forward_scores.maha(to(cuda, f), to(cuda, labels), 4)).all())
