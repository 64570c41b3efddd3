"""Child process of tests/test_gpu_select_class.py: the FIRST dd_select_topk_by_class of a fresh
process captured into a HIP graph on one stream (n = 50 003, 10 classes), replayed three
times, then once more after the keys changed in place; every replay is bit-exact against the
NumPy restatement.  Prints "graph ok".  Not collected by pytest."""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))                    # tests/ (the restatement)
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))   # the repository root


def main():
    import numpy as np
    import torch

    from data_diet_distributed_amd import _capi
    from test_select_policy import ref_quotas, ref_select_by_class

    n, C = 50003, 10
    rng = np.random.default_rng(5)
    keys = rng.random(n, dtype=np.float32)
    labels = rng.integers(0, C, n).astype(np.int64)
    skip, quota = ref_quotas(labels, C, n // 3, "balanced", skip=n // 10)
    k = sum(quota)
    t = torch.from_numpy(keys).cuda()
    y = torch.from_numpy(labels).cuda()
    s_d = torch.tensor(skip, dtype=torch.int64).cuda()
    q_d = torch.tensor(quota, dtype=torch.int64).cuda()
    ws = torch.empty(_capi.select_by_class_workspace_bytes(n, C), dtype=torch.uint8,
                     device="cuda")
    idx = torch.empty(k, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    ref = ref_select_by_class(keys, labels, C, skip, quota)
    stream = torch.cuda.Stream()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=stream):
        _, nan, err = _capi.select_topk_by_class(t, y, C, s_d, q_d, k_total=k, idx_out=idx,
                                                 workspace=ws, check=False)
    for r in range(3):
        idx.fill_(-1)
        g.replay()
        torch.cuda.synchronize()
        got = idx.cpu().numpy()
        assert np.array_equal(got, ref), (r, int((got != ref).sum()), int((got == -1).sum()))
        assert int(nan.item()) == 0 and int(err.item()) == 0
    # the same workspace reused by an eager call
    _capi.select_topk_by_class(t, y, C, s_d, q_d, k_total=k, idx_out=idx, workspace=ws)
    assert np.array_equal(idx.cpu().numpy(), ref), "eager"
    keys2 = keys[::-1].copy()
    t.copy_(torch.from_numpy(keys2))
    idx.fill_(-1)
    g.replay()
    torch.cuda.synchronize()
    assert np.array_equal(idx.cpu().numpy(), ref_select_by_class(keys2, labels, C, skip, quota))
    assert int(nan.item()) == 0 and int(err.item()) == 0
    print("graph ok")
    return 0


if __name__ == "__main__":
    sys.exit(main())
