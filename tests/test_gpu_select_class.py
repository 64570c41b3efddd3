"""Per-class keep-set selection (dd_class_counts, dd_select_topk_by_class) against the NumPy
restatement of the contract in tests/test_select_policy.py.  Integer / index work: every
result is bit-exact (same indices, same order).

Sizes: dd_select_topk tiles by 4096 entries, the class ranking by 2048 (one block per tile up
to 128 blocks: 300 007 entries put two tiles on a block and leave blocks empty); class counts
live in LDS up to 2048 classes and in global memory above.
"""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from data_diet_distributed_amd import _capi
from data_diet_distributed_amd.scoring import apportion
from test_select_policy import ref_quotas, ref_select_by_class

pytestmark = pytest.mark.gpu

SIZES = [1, 10, 2047, 2049, 4095, 4096, 4097, 8191, 50003]
CLASSES = [1, 3, 10, 100, 3000]
GUARD = 64
TIE_VALUES = np.array([0.5, 0.25, 0.0, -0.0, 1.0, 3.0, -2.0], dtype=np.float32)


def _labels(rng, n, C):
    """Skewed class sizes (class c about 1 / (c + 1) of the first class); above 64 classes
    uniform, most classes holding a few members or none."""
    if C > 64:
        return rng.integers(0, C, n).astype(np.int64)
    p = 1.0 / np.arange(1, C + 1)
    return rng.choice(C, size=n, p=p / p.sum()).astype(np.int64)


def _run(cuda, keys, labels, C, skip, quota, check=True):
    """The kept indices (NumPy), with a guard of -1 after idx_out[k_total) checked."""
    k = int(np.sum(quota))
    buf = torch.full((k + GUARD,), -1, dtype=torch.int64, device=cuda)
    t = torch.from_numpy(np.asarray(keys, dtype=np.float32)).to(cuda)
    y = torch.from_numpy(np.asarray(labels, dtype=np.int64)).to(cuda)
    try:
        idx, nan, err = _capi.select_topk_by_class(t, y, C, list(skip), list(quota),
                                                   idx_out=buf[:k], check=check)
    finally:
        torch.cuda.synchronize()
        assert bool((buf[k:] == -1).all()), "written past idx_out[k_total)"
    return idx.cpu().numpy(), int(nan.item()), int(err.item())


def _windows(rng, labels, C):
    """(name, skip, quota) cases for one label set: both rules with and without a skip, the
    ends k = 0, k = N and skip + k = N, and random windows with empty and full classes."""
    n = len(labels)
    n_c = np.bincount(labels, minlength=C)
    out = [("stratified k=n/2", *ref_quotas(labels, C, n // 2, "stratified")),
           ("balanced k=n/3", *ref_quotas(labels, C, n // 3, "balanced")),
           ("stratified skip", *ref_quotas(labels, C, n // 4, "stratified", skip=n // 5)),
           ("balanced skip", *ref_quotas(labels, C, n // 4, "balanced", skip=n // 5)),
           ("k=0", [0] * C, [0] * C),
           ("k=N", [0] * C, n_c.tolist()),
           ("skip+k=N", *ref_quotas(labels, C, n - n // 3, "stratified", skip=n // 3))]
    s = rng.integers(0, n_c + 1)
    q = rng.integers(0, n_c - s + 1)
    mode = rng.integers(0, 3, C)  # a third of the classes keep nothing, a third everything
    q = np.where(mode == 0, 0, q)
    s = np.where(mode == 1, 0, s)
    q = np.where(mode == 1, n_c, q)
    out.append(("random windows", s.tolist(), q.tolist()))
    return out


@pytest.mark.parametrize("n", SIZES)
def test_select_by_class_sizes(cuda, n):
    rng = np.random.default_rng(n)
    keys = rng.random(n, dtype=np.float32)
    for C in CLASSES:
        labels = _labels(rng, n, C)
        for name, skip, quota in _windows(rng, labels, C):
            got, nan, err = _run(cuda, keys, labels, C, skip, quota)
            want = ref_select_by_class(keys, labels, C, skip, quota)
            assert nan == 0 and err == 0
            assert np.array_equal(got, want), (n, C, name)


def test_select_by_class_two_tiles_per_block(cuda):
    # 147 ranking tiles over 128 blocks: two tiles per block (the in-class ranks run on across
    # a block's tiles), the blocks past the 74th empty
    n = 300007
    rng = np.random.default_rng(5)
    keys = rng.random(n, dtype=np.float32)
    for C in (10, 3000):
        labels = _labels(rng, n, C)
        for policy, skip in (("balanced", 0), ("stratified", n // 7)):
            s, q = ref_quotas(labels, C, n // 2, policy, skip)
            got, _, err = _run(cuda, keys, labels, C, s, q)
            assert err == 0
            assert np.array_equal(got, ref_select_by_class(keys, labels, C, s, q)), (C, policy)


def test_select_by_class_more_classes_than_examples(cuda):
    n, C = 20011, 70000
    rng = np.random.default_rng(11)
    keys = rng.random(n, dtype=np.float32)
    labels = rng.integers(0, C, n).astype(np.int64)
    for policy, skip in (("stratified", 0), ("balanced", 0), ("balanced", 1000)):
        s, q = ref_quotas(labels, C, n // 2, policy, skip)
        got, _, err = _run(cuda, keys, labels, C, s, q)
        assert err == 0
        assert np.array_equal(got, ref_select_by_class(keys, labels, C, s, q)), (policy, skip)
    counts, bad = _capi.class_counts(torch.from_numpy(labels).to(cuda), C)
    assert int(bad.item()) == 0
    assert np.array_equal(counts.cpu().numpy(), np.bincount(labels, minlength=C))


@pytest.mark.parametrize("C", [1, 3, 10, 100, 3000])
def test_select_by_class_heavy_ties(cuda, C):
    # seven distinct values (+0.0 and -0.0 tie) over 10 000 keys: ties within and across classes
    rng = np.random.default_rng(C)
    keys = TIE_VALUES[rng.integers(0, len(TIE_VALUES), 10000)]
    labels = _labels(rng, len(keys), C)
    for name, skip, quota in _windows(rng, labels, C):
        got, _, err = _run(cuda, keys, labels, C, skip, quota)
        assert err == 0
        assert np.array_equal(got, ref_select_by_class(keys, labels, C, skip, quota)), name


def test_select_by_class_all_equal(cuda):
    n, C = 5000, 7
    rng = np.random.default_rng(2)
    keys = np.full(n, 0.7, np.float32)
    labels = _labels(rng, n, C)
    s, q = ref_quotas(labels, C, 1234, "balanced", skip=100)
    got, _, _ = _run(cuda, keys, labels, C, s, q)
    assert np.array_equal(got, ref_select_by_class(keys, labels, C, s, q))
    assert np.array_equal(got, np.sort(got))  # all tied: ascending index


def test_select_by_class_special_values(cuda):
    keys = np.array([np.inf, -np.inf, 1e-45, -1e-45, 3.4e38, -3.4e38, 0.0, 1.0, 1.0, 2.0,
                     -0.0, 1e-39, -1e-39, np.inf, -np.inf, -3.4e38], dtype=np.float32)
    labels = np.array([0, 1, 0, 1, 2, 2, 0, 1, 2, 0, 1, 2, 0, 1, 2, 0])
    n_c = np.bincount(labels, minlength=3)
    for k in range(len(keys) + 1):
        for policy in ("stratified", "balanced"):
            s, q = ref_quotas(labels, 3, k, policy)
            got, _, _ = _run(cuda, keys, labels, 3, s, q)
            assert np.array_equal(got, ref_select_by_class(keys, labels, 3, s, q)), (k, policy)
    for s0 in range(int(n_c[0]) + 1):  # every window position of class 0
        s, q = [s0, 1, 2], [int(n_c[0]) - s0, 2, 1]
        got, _, _ = _run(cuda, keys, labels, 3, s, q)
        assert np.array_equal(got, ref_select_by_class(keys, labels, 3, s, q)), s0


def test_select_by_class_nan(cuda):
    keys = np.array([1.0, np.nan, 0.5, 2.0, -np.inf, 0.25], dtype=np.float32)
    labels = np.array([0, 1, 1, 0, 1, 1])
    with pytest.raises(ValueError, match="NaN"):
        _run(cuda, keys, labels, 2, [0, 0], [1, 2])
    # unchecked: the NaN ranks last in its class (below -inf) and is counted once
    got, nan, err = _run(cuda, keys, labels, 2, [0, 0], [2, 4], check=False)
    assert nan == 1 and err == 0 and got.tolist() == [3, 0, 2, 5, 4, 1]
    got, nan, err = _run(cuda, keys, labels, 2, [0, 3], [0, 1], check=False)
    assert nan == 1 and err == 0 and got.tolist() == [1]
    # ... also at a size with several blocks, the NaN among the last n % 4 keys
    rng = np.random.default_rng(9)
    n, C = 50003, 10
    keys = rng.random(n, dtype=np.float32)
    keys[-2] = np.nan
    labels = _labels(rng, n, C)
    n_c = np.bincount(labels, minlength=C).tolist()
    got, nan, err = _run(cuda, keys, labels, C, [0] * C, n_c, check=False)
    assert nan == 1 and err == 0 and got[-1] == n - 2
    assert np.array_equal(got, ref_select_by_class(keys, labels, C, [0] * C, n_c))


@pytest.mark.parametrize("n", [1, 10, 4097, 50003])
def test_one_class_without_skip_is_select_topk(cuda, n):
    rng = np.random.default_rng(n + 1)
    for keys in (rng.random(n, dtype=np.float32), TIE_VALUES[rng.integers(0, 7, n)]):
        t = torch.from_numpy(keys).to(cuda)
        y = torch.zeros(n, dtype=torch.int64, device=cuda)
        for k in sorted({0, 1, n // 2, n}):
            a = _capi.select_topk_by_class(t, y, 1, [0], [k])[0]
            b = _capi.select_topk(t, k)[0]
            assert torch.equal(a, b), (n, k)


def test_select_by_class_errors(cuda):
    rng = np.random.default_rng(4)
    n, C = 5000, 10
    keys = rng.random(n, dtype=np.float32)
    labels = _labels(rng, n, C)
    n_c = np.bincount(labels, minlength=C)
    s, q = ref_quotas(labels, C, n // 2, "stratified")
    for bad_label in (C, -1):
        lab = labels.copy()
        lab[n // 2] = bad_label
        with pytest.raises(_capi.LabelError):
            _run(cuda, keys, lab, C, s, q)  # (its finally checks the guard)
        _, _, err = _run(cuda, keys, lab, C, s, q, check=False)
        assert err >= 1
        with pytest.raises(_capi.LabelError):
            _capi.class_counts(torch.from_numpy(lab).to(cuda), C)
        counts, bad = _capi.class_counts(torch.from_numpy(lab).to(cuda), C, check=False)
        assert int(bad.item()) == 1
        want = n_c.copy()
        want[labels[n // 2]] -= 1
        assert np.array_equal(counts.cpu().numpy(), want)
    # a window past the end of its class: idx_out holds only k_total entries
    q_bad = list(q)
    q_bad[3] = int(n_c[3]) + 1
    with pytest.raises(ValueError, match="exceeds"):
        _run(cuda, keys, labels, C, s, q_bad)
    s_bad = [0] * C
    s_bad[C - 1] = int(n_c[C - 1]) - q[C - 1] + 1
    with pytest.raises(ValueError, match="exceeds"):
        _run(cuda, keys, labels, C, s_bad, q)
    # quotas that keep more than k_total entries: nothing lands past idx_out[k_total)
    k = 100
    buf = torch.full((k + GUARD,), -1, dtype=torch.int64, device=cuda)
    with pytest.raises(ValueError):
        _capi.select_topk_by_class(torch.from_numpy(keys).to(cuda),
                                   torch.from_numpy(labels).to(cuda), C, [0] * C, n_c.tolist(),
                                   k_total=k, idx_out=buf[:k])
    torch.cuda.synchronize()
    assert bool((buf[k:] == -1).all())
    with pytest.raises(ValueError):
        _capi.select_topk_by_class(torch.from_numpy(keys).to(cuda),
                                   torch.from_numpy(labels).to(cuda), C, [0] * (C - 1), q)


@pytest.mark.parametrize("n,C", [(1, 1), (10, 3), (4097, 10), (8191, 100), (50003, 3000),
                                 (50003, 10), (300007, 2048), (300007, 2049)])
def test_class_counts(cuda, n, C):
    labels = _labels(np.random.default_rng(n + C), n, C)
    counts, bad = _capi.class_counts(torch.from_numpy(labels).to(cuda), C)
    assert int(bad.item()) == 0
    assert np.array_equal(counts.cpu().numpy(), np.bincount(labels, minlength=C))
    assert apportion(n, counts.tolist(), "balanced") == counts.tolist()


def test_select_by_class_empty(cuda):
    t = torch.empty(0, device=cuda)
    y = torch.empty(0, dtype=torch.int64, device=cuda)
    idx, nan, err = _capi.select_topk_by_class(t, y, 3, [0, 0, 0], [0, 0, 0])
    assert idx.numel() == 0 and int(nan.item()) == 0 and int(err.item()) == 0
    counts, bad = _capi.class_counts(y, 3)
    assert counts.cpu().tolist() == [0, 0, 0] and int(bad.item()) == 0


def test_select_by_class_is_graph_capturable():
    # no entry point allocates or synchronises: the first call of a fresh process, captured on
    # one stream, replays bit-exactly, also after the keys change in place
    # (tests/helpers/select_class_graph_child.py)
    here = os.path.dirname(os.path.abspath(__file__))
    child = os.path.join(here, "helpers", "select_class_graph_child.py")
    r = subprocess.run([sys.executable, child], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "graph ok" in r.stdout, r.stdout[-2000:] + r.stderr[-3000:]
