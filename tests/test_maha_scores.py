"""The maha score on the host: a float64 NumPy restatement of include/dd_capi.h's definition, the
bounds the GPU tests hold the kernels to, and the method / config surface.

    mu_c = proto's class mean (2^-24 fixed-point sums, rounded to fp32); a_i = f_i - mu_{y_i} in
    fp32 (zeros for a class's only row); S = sum_i a_i a_i^T; Sigma = S / N + lambda (tr(S / N) /
    D) I = L L^T; W = L^-1; maha_i = || W a_i ||_2.

With u = 2^-24 and e_op = E_OP[operands] (tests/test_nn_scores.py: what a split product drops):

The scatter bound.  S_kl is a sum over the rows of products a_ik a_il.  Each split product is
within e_op |a_ik a_il| of exact; a segment's fp32 accumulation of n_seg terms in any order adds
at most n_seg u sum |a_ik a_il|; the partial's own store and the float64 sum over the segments
are charged "+ 2 u".  So | S_kl - S64_kl | <= (e_op + (n_seg + 2) u) sum_i |a_ik| |a_il|.

The distance bound, for a given W.  y_j = sum_k W_jk a_k likewise: | y_j - y64_j | <= e_j = (e_op
+ (D + 2) u) (|W| |a|)_j, the "+ 2 u" covering W's rounding to fp32.  Then | y_j^2 - y64_j^2 | <=
2 |y64_j| e_j + e_j^2, and the fp32 sum of the D non-negative squares (each rounded once, at most
D - 1 additions), the square root's rounding and its squaring back add (D + 4) u relative:
    | maha^2 - maha64^2 | <= sum_j (2 |y64_j| e_j + e_j^2) + (D + 4) u sum_j (|y64_j| + e_j)^2.

The whitening bound (the engine test: W itself comes from the device's S).  With E = S - S64 and z =
Sigma^-1 a, a^T (Sigma + dSigma)^-1 a - a^T Sigma^-1 a = - z^T dSigma z to first order, dSigma = E
/ N + lambda (tr(E) / (N D)) I, so the change of maha^2 is at most |z|^T B |z| + lambda (tr(B) / D)
|z|^2 with B the scatter bound / N.  The higher-order terms are charged a factor 2: they are
smaller than the first-order term by ||Sigma^-1 dSigma|| << 1.
"""
import numpy as np
import pytest

from data_diet_distributed_amd import _capi, config, methods
from data_diet_distributed_amd.scoring import ScoreConfig
from test_nn_scores import E_OP

U = 2.0 ** -24


def ref_maha(f, labels, C, shrink):
    """The definition in float64 on rows f fp32 [N, D]: a dict of a [N, D] (the fp32 centred
    rows, as float64), S, W (None without a Cholesky factor), y = W a [N, D] and maha [N]."""
    f, labels = np.asarray(f, np.float32), np.asarray(labels)
    N, D = f.shape
    q = np.rint(f.astype(np.float64) * 2.0 ** 24).astype(np.int64)
    a = np.zeros((N, D), np.float32)
    for c in range(C):
        m = labels == c
        if m.sum() > 1:
            mu = ((q[m].sum(axis=0).astype(np.float64) / m.sum()) * 2.0 ** -24).astype(np.float32)
            a[m] = f[m] - mu
    a = a.astype(np.float64)
    S = a.T @ a
    sigma = S / N + shrink * (np.trace(S / N) / D) * np.eye(D)
    try:
        W = np.tril(np.linalg.inv(np.linalg.cholesky(sigma)))
    except np.linalg.LinAlgError:
        return {"a": a, "S": S, "W": None}
    y = a @ W.T
    return {"a": a, "S": S, "W": W, "y": y, "maha": np.sqrt((y * y).sum(axis=1))}


def scatter_bound(ref, operands, seg_rows):
    return (E_OP[operands] + (seg_rows + 2) * U) * (np.abs(ref["a"]).T @ np.abs(ref["a"]))


def dist_bound(ref, operands):
    """float64 [N]: the bound on | maha^2 - maha64^2 | for the kernel given ref's W."""
    D = ref["a"].shape[1]
    y = np.abs(ref["y"])
    e = (E_OP[operands] + (D + 2) * U) * (np.abs(ref["a"]) @ np.abs(ref["W"]).T)
    return (2 * y * e + e * e).sum(axis=1) + (D + 4) * U * ((y + e) ** 2).sum(axis=1)


def whitening_bound(ref, operands, seg_rows, shrink):
    """float64 [N]: the bound on the change of maha^2 when W is factored from the device's S."""
    N, D = ref["a"].shape
    B = scatter_bound(ref, operands, seg_rows) / N
    z = np.abs(ref["y"] @ ref["W"])  # |Sigma^-1 a| = |W^T W a|
    return 2 * (((z @ B) * z).sum(axis=1) + shrink * np.trace(B) / D * (z * z).sum(axis=1))


def test_method_and_config_surface():
    assert methods.COVARIANCE_METHODS == ("maha",)
    assert methods.known("maha") and methods.pass_of("maha") == "el2n"
    assert not methods.refinable("maha")
    assert config.DEFAULTS["maha_shrink"] == 0.01 == ScoreConfig().maha_shrink
    cfg = ScoreConfig(methods=("maha",), select_by="maha")  # (the parent: unknown score method)
    assert cfg.maha_shrink == 0.01
    assert ScoreConfig(methods=("el2n", "maha"), maha_shrink=1).maha_shrink == 1.0
    for bad in (-0.01, 1.5, True, "0.1", None):
        with pytest.raises(ValueError, match="maha_shrink"):
            ScoreConfig(methods=("maha",), select_by="maha", maha_shrink=bad)
    ScoreConfig(maha_shrink=7)  # validated only when maha is requested
    with pytest.raises(ValueError, match="refine=True"):
        ScoreConfig(methods=("el2n", "maha"), select_by="maha", refine=True)
    assert _capi.lib().dd_abi_version() == 10


def test_entry_points_validate_before_launching():
    """DD_EINVAL and a message before any device work (so this runs without a GPU)."""
    import ctypes
    L, P16 = _capi.lib(), ctypes.c_void_p(16)
    for bad in ((-1, 8, 1), (1 << 31, 8, 1), (4, 0, 1), (4, 4097, 1), (4, 8, 2)):
        assert L.dd_maha_workspace_bytes(*bad) == 0, bad
    assert L.dd_maha_segment_rows(4, 0) == 0 and _capi.maha_segment_rows(1 << 24, 4096) <= 8192

    def scatter(n=4, D=8, C=3, operands=1, rows=P16, S=P16, ws=P16, ws_bytes=1 << 30):
        return L.dd_maha_scatter(rows, P16, P16, P16, n, D, C, operands, S, P16, ws, ws_bytes, None)

    def dist(n=4, D=8, operands=1, W=P16, out=P16, ws=P16, ws_bytes=1 << 30):
        return L.dd_maha_dist(P16, P16, P16, P16, n, D, 3, W, operands, out, None, ws, ws_bytes, None)

    for fn, kw, word in ((scatter, {"D": 0}, b"<= D"), (scatter, {"C": 0}, b"<= C"),
                         (scatter, {"operands": 2}, b"operands"), (scatter, {"S": None}, b"null"),
                         (scatter, {"rows": None}, b"null"), (scatter, {"ws_bytes": 64}, b"workspace"),
                         (scatter, {"ws": ctypes.c_void_p(24)}, b"aligned"),
                         (dist, {"D": 4097}, b"<= D"), (dist, {"n": 1 << 31}, b"<= n"),
                         (dist, {"out": None}, b"no output"), (dist, {"W": None}, b"null"),
                         (dist, {"ws": None}, b"workspace")):
        assert fn(**kw) == -1, kw
        err = L.dd_last_error()
        assert err.startswith(b"dd_maha_" + fn.__name__.encode()) and word in err, (kw, err)
    assert dist(n=0, ws=None, ws_bytes=0) == 0 and L.dd_last_error() == b""
