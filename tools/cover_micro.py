"""Timing of the ball-cover fill (dd_cover_greedy) at the CIFAR-10 `stratified` shape: G groups of
NG rows, D columns, one seed per group, quotas of NG / 2 (DESIGN 4.17's table).  Run alone on the
device:

    python tools/cover_micro.py [G NG D]

Prints one JSON object: (median, min, max) seconds of the call with no picks (sort, pack, the
matrices, the means, P, theta, the bits and the seeds' cover) and of the call with NG / 2 - 1 picks
per group at two radii, the select kernel's time as their difference, the time per pick, the
coverage reached, and dd_herding_greedy's and dd_kmedoids_greedy's calls on the same inputs (the
same matrices; the inertia fill with 64 picks, its cost per pick being flat) for comparison.
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
    prio = (torch.arange(n, dtype=torch.int32) // G).to(dev)  # a row's place in its group
    sizes, m = [ng] * G, [1] * G

    def cover(p, radius):
        return _capi.cover_greedy(rows, None, groups, sizes, seeds, m, [p] * G, prio, radius,
                                  check=False)

    picks = ng // 2 - 1
    res = {"shape": [G, ng, D], "picks": picks}
    res["cover_no_picks"] = timed(lambda: cover(0, 0.25), 15)
    for radius in (0.25, 0.9):
        key = f"cover_r{radius}"
        res[key + "_full"] = timed(lambda: cover(picks, radius), 15)
        select = res[key + "_full"][0] - res["cover_no_picks"][0]
        res[key + "_select_ms"] = select * 1e3
        res[key + "_per_pick_us"] = select / picks * 1e6  # (the ten groups pick side by side)
        _, gain, (_, covered), _ = cover(picks, radius)
        res[key + "_coverage"] = float(covered.sum()) / n
        res[key + "_picks_with_gain"] = int((gain[:, 0] > 0).sum())
    for name, fn in (("herding", _capi.herding_greedy), ("kmedoids", _capi.kmedoids_greedy)):
        p = picks if name == "herding" else 64
        res[name + "_no_picks"] = timed(lambda: fn(rows, None, groups, sizes, seeds, m, [0] * G,
                                                   check=False), 15)
        res[name + "_full"] = timed(lambda: fn(rows, None, groups, sizes, seeds, m, [p] * G,
                                               check=False), 15 if name == "herding" else 3)
        res[name + "_per_pick_us"] = (res[name + "_full"][0] - res[name + "_no_picks"][0]) / p * 1e6
    print(json.dumps(res, indent=1))


if __name__ == "__main__":
    main(*(int(v) for v in sys.argv[1:4]))
