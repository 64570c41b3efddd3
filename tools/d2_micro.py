"""Timing of the D2 selection (dd_knn, dd_d2_weights, dd_d2_propagate, dd_d2_select) at the
CIFAR-10 shape: N rows of D columns, k neighbours, one group, keeping KEEP of them (DESIGN 4.14's
table).  Run alone on the device:

    python tools/d2_micro.py [N D K KEEP]

Prints one JSON object: (median, min, max) seconds of every stage, each a host clock around the
call and a device synchronise; the select with no picks (its init launch and the tables) and the
microseconds per pick derived from the two; the score cut (dd_select_topk) and the radius fill
(dd_kcenter_greedy, one seed) at the same shape as context; and the cost of a launch on this
machine: the smallest launch the library has (dd_d2_weights on one slot: one workgroup, one
thread at work), LAUNCHES of them back to back on the stream, per launch.
"""
import ctypes
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from data_diet_distributed_amd import _capi  # noqa: E402

LAUNCHES = 20000


def timed(fn, reps):
    fn()  # warm-up
    torch.cuda.synchronize()
    out = []
    for _ in range(reps):
        t = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        out.append(time.perf_counter() - t)
    return float(np.median(out)), float(min(out)), float(max(out))


def main(n=50000, D=512, k=10, keep=25000):
    dev = torch.device("cuda:0")
    gen = torch.Generator(device="cpu").manual_seed(0)
    rows = (torch.randn((n, D), generator=gen).clamp(min=0) + 0.5).to(dev)
    keys = torch.rand(n, generator=gen).to(dev)
    ids = torch.arange(n, dtype=torch.int64, device=dev)
    dist = torch.empty((n, k), dtype=torch.float32, device=dev)
    nbr = torch.empty((n, k), dtype=torch.int64, device=dev)
    ws = torch.empty(_capi.knn_workspace_bytes(n, n, D, k), dtype=torch.uint8, device=dev)

    res = {"shape": [n, D, k, keep]}
    res["knn"] = timed(lambda: _capi.knn(rows, ids, rows, ids, k, dist=dist, nbr_id=nbr,
                                         workspace=ws), 5)
    coef = float(np.float32(1.0 / (dist.double() ** 2).mean().item()))
    w = torch.empty_like(dist)
    res["weights"] = timed(lambda: _capi.d2_weights(dist, nbr, coef, w=w), 15)
    res["propagate"] = timed(lambda: _capi.d2_propagate(keys, nbr, w, check=False), 15)
    x1 = _capi.d2_propagate(keys, nbr, w)[0]
    res["select_no_picks"] = timed(lambda: _capi.d2_select(x1, nbr, w, [0], check=False), 15)
    res["select"] = timed(lambda: _capi.d2_select(x1, nbr, w, [keep], check=False), 7)
    res["per_pick_us"] = (res["select"][0] - res["select_no_picks"][0]) / keep * 1e6
    # context: the rank cut and the radius fill at the same shape
    res["score_cut"] = timed(lambda: _capi.select_topk(keys, keep, check_nan=False), 15)
    seed = torch.zeros(1, dtype=torch.int64, device=dev)
    res["radius_fill"] = timed(lambda: _capi.kcenter_greedy(rows, None, None, [n], seed, [1],
                                                            [keep - 1], check=False), 3)
    res["radius_per_pick_us"] = res["radius_fill"][0] / (keep - 1) * 1e6
    # a launch: the one-slot dd_d2_weights, straight through the C entry
    L, one = _capi.lib(), ctypes.c_void_p
    args = (one(dist.data_ptr()), one(nbr.data_ptr()), 1, 1, ctypes.c_float(coef),
            one(w.data_ptr()), one(torch.cuda.current_stream(dev).cuda_stream))

    def launches():
        for _ in range(LAUNCHES):
            L.dd_d2_weights(*args)

    res["launch_us"] = timed(launches, 5)[0] / LAUNCHES * 1e6
    print(json.dumps(res, indent=1))


if __name__ == "__main__":
    main(*(int(v) for v in sys.argv[1:5]))
