"""The logit scores beside EL2N (dd_logit_scores): the NumPy float64 restatement of the six
statistics (the reference the GPU tests compare with), the host-side surface (ScoreConfig,
config mapping, exported symbols) and the entry point's argument checks, all without a GPU.
"""
import ctypes

import numpy as np
import pytest

from data_diet_distributed_amd import _capi, score
from data_diet_distributed_amd.scoring import LOGIT_FAMILY, LOGIT_METHODS, ScoreConfig

STATS = ("loss", "margin", "entropy", "error", "wrong_mass")
# the project's kernel tolerance (tests/test_gpu_kernels.py: RTOL and the atol of its calls)
RTOL, ATOL = 1e-3, 1e-6


def ref_logit_stats(logits, labels):
    """{statistic: float64 [B]} of fp32 (or float64) logits [B, C] and labels [B], by the
    formulas of include/dd_capi.h in float64.  A row with a NaN or +inf logit, or a label
    outside [0, C), is NaN in every statistic."""
    z = np.asarray(logits, dtype=np.float64)
    y = np.asarray(labels, dtype=np.int64)
    B, C = z.shape
    bad = (y < 0) | (y >= C) | ~(z < np.inf).all(axis=1)
    yc = np.where(bad, 0, y)
    zz = np.where(bad[:, None], 0.0, z)
    onehot = np.arange(C)[None, :] == yc[:, None]
    m = zz.max(axis=1)
    d = zz - m[:, None]
    e = np.exp(d)
    s = e.sum(axis=1)
    zy = zz[np.arange(B), yc]
    mo = np.where(onehot, -np.inf, zz).max(axis=1) if C > 1 else np.full(B, -np.inf)
    with np.errstate(invalid="ignore"):
        t = np.where(e > 0, e * d, 0.0).sum(axis=1)  # a term with e_j == 0 contributes 0
        out = {"loss": (m - zy) + np.log(s),
               "margin": mo - zy,
               "entropy": np.log(s) - t / s,
               "error": (mo >= zy).astype(np.float64),
               "wrong_mass": np.where(onehot, 0.0, e).sum(axis=1) / s}
    for v in out.values():
        v[bad] = np.nan
    return out


def ref_variability(wrong_mass_per_ckpt):
    """Population standard deviation (ddof 0) of wrong_mass [K, B] over the K checkpoints."""
    return np.std(np.asarray(wrong_mass_per_ckpt, dtype=np.float64), axis=0)


def ref_ensemble(logit_sets, labels):
    """{method: float64 [B]} over K logit sets: the mean of the five statistics + variability."""
    per = [ref_logit_stats(z, labels) for z in logit_sets]
    out = {m: np.mean([p[m] for p in per], axis=0) for m in STATS}
    out["variability"] = ref_variability([p["wrong_mass"] for p in per])
    return out


# ---- the restatement against hand-computed rows ----------------------------------------------
def test_restatement_plain_row():
    # p = (1/4, 3/4), label 0
    r = ref_logit_stats(np.array([[0.0, np.log(3.0)]]), [0])
    assert r["loss"][0] == pytest.approx(np.log(4.0), rel=1e-14)
    assert r["margin"][0] == pytest.approx(np.log(3.0), rel=1e-14)
    assert r["entropy"][0] == pytest.approx(-(0.25 * np.log(0.25) + 0.75 * np.log(0.75)),
                                            rel=1e-14)
    assert r["error"][0] == 1.0
    assert r["wrong_mass"][0] == pytest.approx(0.75, rel=1e-14)
    r = ref_logit_stats(np.array([[0.0, np.log(3.0)]]), [1])
    assert r["loss"][0] == pytest.approx(np.log(4.0 / 3.0), rel=1e-14)
    assert r["margin"][0] == pytest.approx(-np.log(3.0), rel=1e-14)
    assert r["error"][0] == 0.0
    assert r["wrong_mass"][0] == pytest.approx(0.25, rel=1e-14)


def test_restatement_all_tie_row():
    # a tie with the label is an error (not "argmax picks the first index"), margin 0
    for y in range(4):
        r = ref_logit_stats(np.full((1, 4), 1.0, np.float32), [y])
        assert r["error"][0] == 1.0 and r["margin"][0] == 0.0
        assert r["loss"][0] == pytest.approx(np.log(4.0), rel=1e-14)
        assert r["entropy"][0] == pytest.approx(np.log(4.0), rel=1e-14)
        assert r["wrong_mass"][0] == pytest.approx(0.75, rel=1e-14)


def test_restatement_saturated_rows():
    z = np.zeros((2, 3), np.float32)
    z[:, 0] = 1e4
    r = ref_logit_stats(z, [0, 1])
    assert all(np.isfinite(v).all() for v in r.values())
    assert r["loss"].tolist() == [0.0, 1e4]
    assert r["entropy"].tolist() == [0.0, 0.0]
    assert r["wrong_mass"].tolist() == [0.0, 1.0]
    assert r["margin"].tolist() == [-1e4, 1e4]
    assert r["error"].tolist() == [0.0, 1.0]


def test_restatement_nan_rules():
    z = np.zeros((4, 3), np.float32)
    z[1, 2] = np.nan
    z[2, 0] = np.inf
    r = ref_logit_stats(z, [0, 0, 1, 3])  # clean, NaN logit, +inf logit, bad label
    for v in r.values():
        assert np.isfinite(v[0]) and np.isnan(v[1:]).all()


def test_restatement_variability():
    rng = np.random.default_rng(0)
    z = rng.normal(size=(1, 5, 4))
    assert ref_ensemble(z, [0, 1, 2, 3, 0])["variability"].tolist() == [0.0] * 5  # K = 1
    w = np.array([[0.25], [0.75]])
    assert ref_variability(w)[0] == 0.25
    assert ref_variability(np.full((7, 3), 0.3)).tolist() == [0.0] * 3


# ---- the host-side surface -------------------------------------------------------------------
def test_score_config_accepts_the_family():
    assert LOGIT_METHODS == STATS + ("variability",)
    assert LOGIT_FAMILY == ("el2n",) + LOGIT_METHODS
    c = ScoreConfig(methods=LOGIT_FAMILY + ("grand",), select_by="entropy")
    assert c.methods == LOGIT_FAMILY + ("grand",)
    for m in LOGIT_METHODS:
        assert ScoreConfig(methods=(m,), select_by=m).select_by == m
    with pytest.raises(ValueError, match="refine"):
        ScoreConfig(methods=("el2n", "margin"), select_by="margin", refine=True)
    ScoreConfig(methods=("el2n", "margin"), select_by="el2n", refine=True)
    with pytest.raises(ValueError, match="unknown score method"):
        ScoreConfig(methods=("foo",))
    with pytest.raises(ValueError):
        ScoreConfig(methods=("el2n",), select_by="loss")


def test_engine_config_maps_the_new_names():
    cfg = {"batch_size": 128, "score_methods": ["el2n", "loss", "variability"],
           "select_by": "loss"}
    ec = score.engine_config(cfg)
    assert ec.methods == ("el2n", "loss", "variability") and ec.select_by == "loss"
    assert score.engine_config({"batch_size": 128, "score_methods": "margin"}).select_by == \
        "margin"


def test_new_symbols_are_exported():
    for name in ("dd_logit_scores", "dd_variability_finalize"):
        assert name in _capi.EXPORTS
        assert hasattr(_capi.lib(), name)
    assert _capi.lib().dd_abi_version() == 10
    assert _capi.LOGIT_STATS == STATS


def test_entry_point_validates_before_launching():
    """Bad arguments are refused with rc -1 and a message before any device work (so this runs
    without a GPU).  Arguments: logits, labels, B, C, loss, margin, entropy, error, wrong_mass,
    var_mean, var_m2, k, bad_labels, stream."""
    L = _capi.lib()
    P16 = ctypes.c_void_p(16)
    f = L.dd_logit_scores

    def refused(rc, word):
        assert rc == -1
        assert word in L.dd_last_error(), L.dd_last_error()

    refused(f(P16, P16, -1, 10, P16, None, None, None, None, None, None, 0, None, None), b"B < 0")
    refused(f(P16, P16, 4, 0, P16, None, None, None, None, None, None, 0, None, None),
            b"C must be positive")
    refused(f(P16, P16, 4, -3, P16, None, None, None, None, None, None, 0, None, None),
            b"C must be positive")
    # margin / error need a second class
    refused(f(P16, P16, 4, 1, None, P16, None, None, None, None, None, 0, None, None), b"C >= 2")
    refused(f(P16, P16, 4, 1, None, None, None, P16, None, None, None, 0, None, None), b"C >= 2")
    # null logits / labels with B > 0
    refused(f(None, P16, 4, 10, P16, None, None, None, None, None, None, 0, None, None), b"null")
    refused(f(P16, None, 4, 10, P16, None, None, None, None, None, None, 0, None, None), b"null")
    # the Welford pair: both pointers, and k >= 1
    refused(f(P16, P16, 4, 10, None, None, None, None, None, P16, None, 1, None, None), b"both")
    refused(f(P16, P16, 4, 10, None, None, None, None, None, None, P16, 1, None, None), b"both")
    refused(f(P16, P16, 4, 10, None, None, None, None, None, P16, P16, 0, None, None), b"k >= 1")
    refused(f(P16, P16, 4, 10, None, None, None, None, None, P16, P16, -2, None, None), b"k >= 1")
    # nothing requested is an error, also at B == 0
    refused(f(P16, P16, 4, 10, None, None, None, None, None, None, None, 0, None, None),
            b"no statistic")
    refused(f(None, None, 0, 10, None, None, None, None, None, None, None, 0, None, None),
            b"no statistic")
    # B == 0 returns cleanly (no buffers needed), with the loss alone or everything
    assert f(None, None, 0, 10, P16, None, None, None, None, None, None, 0, None, None) == 0
    assert f(None, None, 0, 10, P16, P16, P16, P16, P16, P16, P16, 3, None, None) == 0
    assert L.dd_last_error() == b""
    g = L.dd_variability_finalize
    assert g(P16, -1, 2, P16, None) == -1 and b"bad n/K" in L.dd_last_error()
    assert g(P16, 4, 0, P16, None) == -1
    assert g(None, 4, 2, P16, None) == -1 and b"null" in L.dd_last_error()
    assert g(None, 0, 2, None, None) == 0
