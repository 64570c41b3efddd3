"""Timing of the maha score's per-checkpoint steps (DESIGN 4.13's table).  Run alone on the device:

    python tools/maha_micro.py [N D C]

Host clock around windows that end in a synchronise, one warm-up window, then the (median, min,
max) seconds per call over the windows.  A window of a kernel step is BATCH = 20 calls issued back
to back (one call is 0.1 to 4 ms: a window of one would time the clock and the launch as much as
the kernel); a window of the host algebra or of the whole, which synchronise inside, is one call.
The steps: the class means (dd_class_feature_sums + dd_class_centroids), the scatter
(dd_maha_scatter) per operand kind against its 3 * 2 N D^2 / 2 split flop, the host algebra (S to the host, scale,
shrink, float64 Cholesky, triangular inverse, W back), the distance (dd_maha_dist, its two pack
passes included) against the split flop the triangular skip leaves, and all of them in sequence
as forward_scores.maha runs them.  Prints one JSON object.
"""
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from data_diet_distributed_amd import _capi, forward_scores  # noqa: E402


BATCH = 20


def timed(fn, reps, batch=1):
    fn()  # warm-up
    torch.cuda.synchronize()
    out = []
    for _ in range(reps):
        t = time.perf_counter()
        for _ in range(batch):
            fn()
        torch.cuda.synchronize()
        out.append((time.perf_counter() - t) / batch)
    return float(np.median(out)), float(min(out)), float(max(out))


def main(N=50000, D=512, C=10, reps=9):
    dev = torch.device("cuda:0")
    gen = torch.Generator(device="cpu").manual_seed(0)
    scale = torch.linspace(1, 30, D)
    rows = ((torch.randn((N, D), generator=gen).clamp(min=0) + 0.5) * scale).to(dev)
    labels = (torch.arange(N) % C).to(dev)
    counts, _ = _capi.class_counts(labels, C, check=True)
    order = torch.argsort(labels, stable=True)
    mean, _ = forward_scores.class_means(rows, labels, counts, order)
    S, _, ws = _capi.maha_scatter(rows, labels, counts, mean)
    W = forward_scores.maha_whitener(S, N, 0.01)
    dist = torch.empty(N, dtype=torch.float32, device=dev)

    res = {"shape": [N, D, C], "segment_rows": _capi.maha_segment_rows(N, D)}
    res["class_means"] = timed(lambda: forward_scores.class_means(rows, labels, counts, order), reps,
                               BATCH)
    for op in ("f16x3", "bf16x3"):
        res["scatter_" + op] = timed(
            lambda: _capi.maha_scatter(rows, labels, counts, mean, operands=op, out=S,
                                       workspace=ws), reps, BATCH)
        res["dist_" + op] = timed(
            lambda: _capi.maha_dist(rows, labels, counts, mean, W, operands=op, dist=dist,
                                    workspace=ws), reps, BATCH)
    res["host_algebra"] = timed(lambda: forward_scores.maha_whitener(S, N, 0.01), 5)
    res["all_in"] = timed(lambda: forward_scores.maha(rows, labels, C), 5)
    # per 128-output block c0 the K chunks of 64 below min(pad16(D), c0 + 128)
    Dp = (D + 15) // 16 * 16
    ksum = sum(min(Dp, c0 + 128) for c0 in range(0, D, 128))
    res["scatter_split_flop"] = 3.0 * N * D * D
    res["dist_split_flop"] = 3.0 * 2 * N * 128 * ksum
    res["scatter_TFLOPs"] = res["scatter_split_flop"] / res["scatter_f16x3"][0] / 1e12
    res["dist_TFLOPs"] = res["dist_split_flop"] / res["dist_f16x3"][0] / 1e12
    print(json.dumps(res, indent=1))


if __name__ == "__main__":
    main(*(int(v) for v in sys.argv[1:4]))
