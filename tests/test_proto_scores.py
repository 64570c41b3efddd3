"""The prototype-distance score ("proto") on the host: a NumPy restatement of the definition
(float64, the exact class mean), a restatement of the library's fixed-point centroid, the
tolerances the GPU tests hold the kernels to (checked here against plain fp32 NumPy arithmetic on
the GPU tests' own inputs), the config surface, and the entry points' argument checks, which run
before any device work.

    mu_c    = mean of f_i over every example with label c
    proto_i = || f_i - mu_{y_i} ||_2, then the mean over the K checkpoints
"""
import ctypes
import math

import numpy as np
import pytest

from data_diet_distributed_amd import _capi, score as score_mod
from data_diet_distributed_amd.scoring import (FEATURE_METHODS, FORWARD_FAMILY, LOGIT_FAMILY,
                                               LOGIT_METHODS, ScoreConfig, ScoringEngine,
                                               check_class_sizes, pass_of)

SCALE = 2.0 ** 24


# ---- restatement -------------------------------------------------------------------------------
def exact_class_means(f, labels, C):
    """float64 [C, D]: the class means of f [n, D], each the correctly rounded sum (math.fsum)
    divided once; 0 for a class with no member."""
    f = np.asarray(f, np.float64)
    labels = np.asarray(labels)
    mu = np.zeros((C, f.shape[1]), np.float64)
    for c in range(C):
        rows = f[labels == c]
        if len(rows):
            mu[c] = [math.fsum(col) / len(rows) for col in rows.T]
    return mu


def ref_proto(features, labels, C):
    """float64 [n]: the mean over the K feature sets [K, n, D] of the distance of every row to
    its class's exact mean.  A label outside [0, C) gives NaN."""
    features = np.asarray(features)
    labels = np.asarray(labels)
    ok = (labels >= 0) & (labels < C)
    out = np.zeros(features.shape[1], np.float64)
    for f in features:
        f = f.astype(np.float64)
        mu = exact_class_means(f[ok], labels[ok], C)
        d = np.full(len(labels), np.nan)
        d[ok] = np.sqrt(((f[ok] - mu[labels[ok]]) ** 2).sum(axis=1))
        out += d
    return out / len(features)


def ref_class_sums(f, labels, C):
    """int64 [C, D]: the per-class sums of q(v) = rint(v * 2^24).  |q| < 2^39 for |v| < 2^15, so
    with fewer than 2^24 rows the int64 sums are exact: they equal the Python-int sums
    (test_sums_are_python_int_sums)."""
    f = np.asarray(f, np.float32)
    labels = np.asarray(labels)
    assert len(f) < 2 ** 24 and np.all(np.abs(f) < 2.0 ** 15)
    q = np.rint(f.astype(np.float64) * SCALE).astype(np.int64)
    S = np.zeros((C, f.shape[1]), np.int64)
    for c in range(C):
        S[c] = q[labels == c].sum(axis=0, dtype=np.int64)
    return S


def ref_centroid_q(f, labels, C):
    """The library's centroid: fp32 [C, D] = float32(float64(S) / count * 2^-24) of the
    fixed-point sums S; 0 for a class with no member.  Returns (S, centroids)."""
    S = ref_class_sums(f, labels, C)
    cnt = np.bincount(np.asarray(labels), minlength=C)[:C].astype(np.float64)
    cent = np.zeros(S.shape, np.float32)
    has = cnt > 0
    cent[has] = (S[has].astype(np.float64) / cnt[has, None] * 2.0 ** -24).astype(np.float32)
    return S, cent


def dist64(f, labels, cent):
    """float64 distances of the rows of f to the given centroid array."""
    d = np.asarray(f, np.float64) - np.asarray(cent, np.float64)[labels]
    return np.sqrt((d * d).sum(axis=1))


# ---- the tolerances of the GPU tests -------------------------------------------------------------
def bound_same_centroids(D, ref):
    """|got - ref| against float64 on the same fp32 centroid array: D non-negative fp32 terms
    summed in any order plus the per-term roundings stay within D 2^-24 relative; the square
    root halves it."""
    return D * 2.0 ** -24 * np.asarray(ref)


def bound_exact_mean(D, ref, mu_max):
    """... against the exact-mean restatement: additionally every centroid component is off by
    at most the fixed-point step's half (2^-25) plus its fp32 rounding (2^-24 |mu|), and a
    distance moves by at most the norm of its centroid's displacement."""
    return bound_same_centroids(D, ref) + math.sqrt(D) * (2.0 ** -25 + 2.0 ** -24 * mu_max)


def bound_ensemble(D, ref, mu_max, K):
    """... of the K-checkpoint mean: the fp32 running sum and the one division add (K + 1) 2^-24
    relative."""
    return bound_exact_mean(D, ref, mu_max) + (K + 1) * 2.0 ** -24 * np.asarray(ref)


# ---- inputs shared with the GPU tests ----------------------------------------------------------
def make_features(n, D, seed):
    """fp32 [n, D]: signed values with magnitudes log-uniform over 1e-6 .. 1e3."""
    rng = np.random.default_rng(seed)
    mag = 10.0 ** rng.uniform(-6, 3, size=(n, D))
    return (mag * rng.choice([-1.0, 1.0], size=(n, D))).astype(np.float32)


def make_labels(n, C, seed, runs=False):
    """int64 [n]: shuffled, or in long runs (sorted); class C - 1 of C >= 3 has no member."""
    rng = np.random.default_rng(seed + 1)
    top = C - 1 if C >= 3 else C
    lab = rng.integers(0, top, size=n).astype(np.int64)
    return np.sort(lab) if runs else lab


def test_single_member_class_on_the_grid_has_distance_zero():
    f = (np.array([[3, -5, 1 << 20], [7, 9, -11], [1, 1, 1]], np.float64) / SCALE)
    f = f.astype(np.float32)
    labels = np.array([0, 2, 2])
    S, cent = ref_centroid_q(f, labels, 4)
    assert S[0].tolist() == [3, -5, 1 << 20] and S[2].tolist() == [8, 10, -10]
    assert np.array_equal(cent[0], f[0])           # a multiple of 2^-24 survives the round trip
    assert not cent[1].any() and not cent[3].any()  # classes with no member
    assert dist64(f, labels, cent)[0] == 0.0
    r = ref_proto(f[None], labels, 4)               # K = 1
    assert r[0] == 0.0 and r[1] == r[2] > 0
    assert np.isnan(ref_proto(f[None], np.array([0, 4, -1]), 4)[1:]).all()


def test_ensemble_is_the_mean_over_checkpoints():
    f = make_features(40, 7, 3)
    lab = make_labels(40, 5, 3)
    one = [ref_proto(f[None] * s, lab, 5) for s in (1.0, 2.0, 4.0)]
    both = ref_proto(np.stack([f, f * 2, f * 4]), lab, 5)
    np.testing.assert_allclose(both, (one[0] + one[1] + one[2]) / 3, rtol=1e-15)
    np.testing.assert_allclose(one[1], 2 * one[0], rtol=1e-15)


def test_sums_are_python_int_sums():
    f = make_features(50, 5, 8)
    f[7] = 32767.99
    lab = make_labels(50, 4, 8)
    S = ref_class_sums(f, lab, 4)
    for c in range(4):
        for d in range(5):
            want = sum(int(np.rint(np.float64(v) * SCALE)) for v in f[lab == c, d])
            assert int(S[c, d]) == want


@pytest.mark.parametrize("n,D,C", [(300, 63, 10), (300, 512, 10), (256, 2048, 100),
                                   (64, 4096, 2)])
def test_bounds_hold_for_plain_fp32_numpy(n, D, C):
    """The GPU tests' tolerances, met by plain fp32 NumPy arithmetic on their inputs: a bound
    that fp32 itself misses would be wrong, not the kernel."""
    f = make_features(n, D, D)
    lab = make_labels(n, C, D)
    _, cent = ref_centroid_q(f, lab, C)
    d32 = f - cent[lab]
    got = np.sqrt((d32 * d32).sum(axis=1, dtype=np.float32))
    assert got.dtype == np.float32
    same = dist64(f, lab, cent)
    exact = ref_proto(f[None], lab, C)
    mu_max = np.abs(exact_class_means(f, lab, C)).max()
    r1 = np.abs(got - same) / bound_same_centroids(D, same)
    r2 = np.abs(got - exact) / bound_exact_mean(D, exact, mu_max)
    print(f"n={n} D={D}: error / bound = {r1.max():.3g} (same centroids), {r2.max():.3g} (exact)")
    assert r1.max() <= 1 and r2.max() <= 1


# ---- host surface ------------------------------------------------------------------------------
def test_method_families():
    assert LOGIT_METHODS == ("loss", "margin", "entropy", "error", "wrong_mass", "variability")
    assert LOGIT_FAMILY == ("el2n",) + LOGIT_METHODS
    assert FEATURE_METHODS == ("proto",)
    assert FORWARD_FAMILY == LOGIT_FAMILY + FEATURE_METHODS
    assert pass_of("proto") == "el2n" and pass_of("grand") == "grand"
    assert pass_of("el2n") == "el2n" and pass_of("loss") == "el2n"


def test_score_config_accepts_proto():
    assert ScoreConfig(methods=("proto",), select_by="proto").methods == ("proto",)
    for ms in (("el2n", "proto"), ("proto", "grand"), LOGIT_FAMILY + ("proto", "grand")):
        for by in ms:
            assert ScoreConfig(methods=ms, select_by=by).select_by == by
    ScoreConfig(methods=("el2n", "proto"), select_by="proto", select_policy="balanced",
                select_skip=3)
    ScoreConfig(methods=("el2n", "proto"), select_by="el2n", refine=True)
    with pytest.raises(ValueError, match="refine"):
        ScoreConfig(methods=("el2n", "proto"), select_by="proto", refine=True)
    with pytest.raises(ValueError, match="unknown score method"):
        ScoreConfig(methods=("prototype",), select_by="prototype")
    with pytest.raises(ValueError, match="select_by"):
        ScoreConfig(methods=("el2n",), select_by="proto")


def test_auto_refinement_leaves_proto_alone():
    shell = ScoringEngine.__new__(ScoringEngine)
    shell.cfg = ScoreConfig(methods=("el2n", "proto"), select_by="proto",
                            el2n_operands="bf16x3")
    assert not shell._refines("proto") and shell._refines("el2n")
    assert shell._f16_forward("proto") is False
    shell.cfg = ScoreConfig(methods=("el2n", "proto"), select_by="proto")
    assert shell._f16_forward("proto") is True  # the family's forward: redone on bf16 halves


def test_engine_config_maps_the_keys():
    cfg = {"batch_size": 128, "score_methods": ["el2n", "proto"], "select_by": "proto"}
    ecfg = score_mod.engine_config(cfg)
    assert ecfg.methods == ("el2n", "proto") and ecfg.select_by == "proto"
    assert score_mod.engine_config({"batch_size": 64, "score_methods": "proto"}).select_by == \
        "proto"


def test_class_size_limit():
    check_class_sizes((1 << 24) - 1)
    with pytest.raises(ValueError, match="2\\^24"):
        check_class_sizes(1 << 24)


def test_exports_and_abi():
    for name in ("dd_class_feature_sums", "dd_class_centroids", "dd_proto_scores"):
        assert name in _capi.EXPORTS and hasattr(_capi.lib(), name)
    assert _capi.lib().dd_abi_version() == 10  # purely additive
    for name in ("class_feature_sums", "class_centroids", "proto_scores"):
        assert callable(getattr(_capi, name))


def test_entry_points_validate_before_launching():
    """Bad arguments give DD_EINVAL and a message before any device work, and empty inputs
    return DD_OK without a launch (so this runs without a GPU)."""
    L = _capi.lib()
    P16 = ctypes.c_void_p(16)

    def sums(n=4, D=8, C=10, feat=P16):
        return L.dd_class_feature_sums(feat, P16, None, n, D, C, P16, P16, None)

    def cents(C=10, D=8):
        return L.dd_class_centroids(P16, P16, P16, C, D, P16, None)

    def scores(B=4, D=8, C=10, feat=P16, score=P16, accum=None):
        return L.dd_proto_scores(feat, P16, P16, B, D, C, score, accum, None)

    for call, name in ((sums, b"dd_class_feature_sums"), (cents, b"dd_class_centroids"),
                       (scores, b"dd_proto_scores")):
        for kw, word in (({"D": 0}, b"<= D"), ({"D": 4097}, b"<= D"), ({"C": 0}, b"<= C"),
                         ({"C": (1 << 20) + 1}, b"<= C")):
            assert call(**kw) == -1, (name, kw)
            assert L.dd_last_error().startswith(name) and word in L.dd_last_error(), kw
    assert sums(n=-1) == -1 and b"n" in L.dd_last_error()
    assert sums(n=1 << 31) == -1
    assert scores(B=-1) == -1 and scores(B=1 << 31) == -1
    assert sums(feat=None) == -1 and b"null" in L.dd_last_error()
    assert scores(feat=None) == -1 and b"null" in L.dd_last_error()
    assert scores(score=None, accum=None) == -1 and b"no output" in L.dd_last_error()
    assert L.dd_class_feature_sums(P16, P16, None, 4, 8, 10, None, P16, None) == -1
    assert L.dd_class_centroids(P16, None, P16, 10, 8, P16, None) == -1
    # nothing to do: DD_OK, whatever the data pointers
    assert sums(n=0) == 0 and sums(n=0, feat=None) == 0 and L.dd_last_error() == b""
    assert scores(B=0) == 0 and scores(B=0, feat=None, score=None, accum=P16) == 0
