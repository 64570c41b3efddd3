"""Timing of the herding fill (dd_herding_greedy) at the CIFAR-10 `stratified` shape: G groups of
NG rows, D columns, one seed per group, quotas of NG / 2 (DESIGN 4.16's table).  Run alone on the
device:

    python tools/herding_micro.py [G NG D]

Prints one JSON object: (median, min, max) seconds of the call with no picks (sort, pack, the
matrices, the means and P) and of the call with NG / 2 - 1 picks per group, the select kernel's
time as their difference, the time per pick, and dd_kmedoids_greedy's call with no picks on the
same inputs (the same matrices) for comparison.
"""
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from data_diet_distributed_amd import _capi  # noqa: E402
from kmedoids_micro import timed  # noqa: E402


def main(G=10, ng=5000, D=512):
    dev = torch.device("cuda:0")
    n = G * ng
    gen = torch.Generator(device="cpu").manual_seed(0)
    rows = (torch.randn((n, D), generator=gen).clamp(min=0) + 0.5).to(dev)
    groups = (torch.arange(n) % G).to(dev)
    seeds = torch.arange(G, dtype=torch.int64, device=dev)  # row g is in group g
    sizes, m = [ng] * G, [1] * G

    def herd(p):
        return _capi.herding_greedy(rows, None, groups, sizes, seeds, m, [p] * G, check=False)

    picks = ng // 2 - 1
    res = {"shape": [G, ng, D], "picks": picks}
    res["herding_no_picks"] = timed(lambda: herd(0), 15)
    res["herding_full"] = timed(lambda: herd(picks), 15)
    res["kmedoids_no_picks"] = timed(lambda: _capi.kmedoids_greedy(
        rows, None, groups, sizes, seeds, m, [0] * G, check=False), 15)
    select = res["herding_full"][0] - res["herding_no_picks"][0]
    res["select_ms"] = select * 1e3
    res["per_pick_us"] = select / picks * 1e6  # (the ten groups pick side by side)
    print(json.dumps(res, indent=1))


if __name__ == "__main__":
    main(*(int(v) for v in sys.argv[1:4]))
