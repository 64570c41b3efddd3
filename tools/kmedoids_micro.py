"""Timing of the inertia fill (dd_kmedoids_greedy) at the CIFAR-10 `stratified` shape: G groups
of NG rows, D columns, one seed per group (DESIGN 4.12's table).  Run alone on the device:

    python tools/kmedoids_micro.py [G NG D]

Prints one JSON object: (median, min, max) seconds of the call with no picks (sort, pack, the
matrices, the seed fold) per operand kind, of the calls with 1 024 picks and with NG / 2 - 1
picks, of the radius fill (dd_kcenter_greedy) on the same inputs, and the per-pick time and
rates derived from them (nominal: sum_g 4 n_g^2 bytes per launch; read: the unkept rows only).
"""
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from data_diet_distributed_amd import _capi  # noqa: E402


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


def main(G=10, ng=5000, D=512):
    dev = torch.device("cuda:0")
    n = G * ng
    gen = torch.Generator(device="cpu").manual_seed(0)
    rows = (torch.randn((n, D), generator=gen).clamp(min=0) + 0.5).to(dev)
    groups = (torch.arange(n) % G).to(dev)
    seeds = torch.arange(G, dtype=torch.int64, device=dev)  # row g is in group g
    sizes, m = [ng] * G, [1] * G

    def km(p, op="f16x3"):
        return _capi.kmedoids_greedy(rows, None, groups, sizes, seeds, m, [p] * G, operands=op,
                                     check=False)

    def kc(p):
        return _capi.kcenter_greedy(rows, None, groups, sizes, seeds, m, [p] * G, check=False)

    few = min(1024, ng // 2 - 1)
    res = {"shape": [G, ng, D]}
    for op in ("f16x3", "bf16x3"):
        res[op + "_no_picks"] = timed(lambda: km(0, op), 15)
    res[f"inertia_{few}_picks"] = timed(lambda: km(few), 7)
    res["inertia_full"] = timed(lambda: km(ng // 2 - 1), 5)
    res["radius_full"] = timed(lambda: kc(ng // 2 - 1), 5)
    res["radius_no_picks"] = timed(lambda: kc(0), 15)
    pick = (res[f"inertia_{few}_picks"][0] - res["f16x3_no_picks"][0]) / few
    res["per_pick_us"] = pick * 1e6
    res["pick_TBps_nominal"] = G * ng * ng * 4 / pick / 1e12
    res["pick_TBps_read"] = sum((ng - 1 - t) * ng * 4 * G for t in range(few)) / few / pick / 1e12
    print(json.dumps(res, indent=1))


if __name__ == "__main__":
    main(*(int(v) for v in sys.argv[1:4]))
