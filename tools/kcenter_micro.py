"""Device-event times of the kcenter fill (profiles/kcenter/kernels_micro.txt):

    python tools/kcenter_micro.py [--n 50000] [--d 512] [--k 25000] [--torch-steps 300]
    python tools/kcenter_micro.py --k 3001 --torch-steps 0 --only global \
        --blocks 0,256,512,1024,2048,4096        (profiles/kcenter/blocks_sweep.txt: a short
    python tools/kcenter_micro.py --k 30010 --torch-steps 0 --only classes \
        --blocks 0,50,102,205,410                 selection, every row still live at each step)

50 000 x 512 rows, k = 25 000, seed fraction 0 and 0.1, as one group ("global") and as ten
balanced classes.  Per configuration, through _capi.kcenter_greedy (the sorting copy included):
the seed phase (the same call with no picks: init + the seed launches), the whole selection, and
from their difference the time per pick step (one launch that folds the newest centre of every
open group and publishes the next).  Two yardsticks:

  the traffic floor  a pick step streams the n D 4 bytes of the rows once (fewer as rows are
                     kept: a kept row is not read again).  102 MB stay inside the 256 MiB
                     Infinity Cache between two steps, so the floor lies between the HBM rate
                     (6.3 TB/s achievable) and the rate of a resident table of that size
                     (7.4-7.9 TB/s measured for 151 MB of rows).
  the torch loop     what a user would otherwise write, in this process on the same rows:
                     difference, square-sum, minimum, argmax per step, no host sync, timed over
                     --torch-steps steps of the global set and of one 5 000-row class.
"""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from data_diet_distributed_amd import _capi  # noqa: E402
from data_diet_distributed_amd.methods import seed_counts  # noqa: E402

HBM_TBS, L3_TBS = 6.3, 7.65


def timed(fn, reps=1):
    fn()  # warm
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(reps + 1)]
    ev[0].record()
    for i in range(reps):
        fn()
        ev[i + 1].record()
    torch.cuda.synchronize()
    return min(ev[i].elapsed_time(ev[i + 1]) for i in range(reps))  # ms


def torch_loop(rows, seeds, steps):
    """Farthest-first in plain torch on one group: no host sync inside."""
    mind = torch.full((rows.shape[0],), float("inf"), device=rows.device)
    for s in seeds.unbind(0):
        mind = torch.minimum(mind, (rows - rows.index_select(0, s.view(1))).square().sum(1))
    mind[seeds] = -1.0
    picked = torch.empty(steps, dtype=torch.int64, device=rows.device)
    for t in range(steps):
        c = torch.argmax(mind).view(1)
        picked[t:t + 1] = c
        mind = torch.minimum(mind, (rows - rows.index_select(0, c)).square().sum(1))
        mind[c] = -1.0
    return picked


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=50000)
    ap.add_argument("--d", type=int, default=512)
    ap.add_argument("--k", type=int, default=25000)
    ap.add_argument("--classes", type=int, default=10)
    ap.add_argument("--torch-steps", type=int, default=300, help="0: skip the torch loop")
    ap.add_argument("--blocks", default="0", help="workgroups per group, comma-separated "
                                                  "(0: the library's choice)")
    ap.add_argument("--only", default="both", choices=("both", "global", "classes"))
    a = ap.parse_args()
    block_list = [int(b) for b in a.blocks.split(",")]
    dev = torch.device("cuda:0")
    n, D, k, C = a.n, a.d, a.k, a.classes
    g = torch.Generator(device=dev).manual_seed(1)
    rows = torch.randn((n, D), generator=g, device=dev).clamp_(min=0).add_(0.5)
    keys = torch.rand(n, generator=g, device=dev)
    labels = (torch.arange(n, device=dev) % C)[torch.randperm(n, generator=g, device=dev)]
    step_mb = n * D * 4 / 1e6
    print(f"n={n} D={D} k={k}: a pick step streams at most {step_mb:.1f} MB = "
          f"{step_mb / HBM_TBS:.1f} us at {HBM_TBS} TB/s (HBM), {step_mb / L3_TBS:.1f} us at "
          f"{L3_TBS} TB/s (a resident table)")
    configs = (("global", None, [n], [k]),
               (f"{C} balanced classes", labels, [n // C] * C, [k // C] * C))
    configs = [c for c, tag in zip(configs, ("global", "classes")) if a.only in ("both", tag)]
    for name, groups, sizes, quotas in configs:
        for frac, blocks in [(f, b) for b in block_list
                             for f in ((0.0, 0.1) if len(block_list) == 1 else (0.0,))]:
            m = seed_counts(quotas, frac)
            if groups is None:
                seeds = _capi.select_topk(keys, m[0])[0]
            else:
                seeds = _capi.select_topk_by_class(keys, groups, C, [0] * C, m)[0]
            picks = [q - s for q, s in zip(quotas, m)]
            run = lambda p: _capi.kcenter_greedy(rows, None, groups, sizes, seeds, m, p,  # noqa
                                                 blocks=blocks)
            seed_ms = timed(lambda: run([0] * len(picks)), reps=3)
            whole_ms = timed(lambda: run(picks), reps=2)
            steps = max(picks)
            us = (whole_ms - seed_ms) * 1e3 / steps
            hbm_us, l3_us = step_mb / HBM_TBS, step_mb / L3_TBS
            near = "neither floor: above twice the HBM one" if us > 2 * hbm_us else (
                "the HBM floor" if abs(us - hbm_us) <= abs(us - l3_us) else
                "the resident-table floor")
            print(f"  {name}, seed_frac={frac}, blocks={blocks}: seeds/group {m[0]}, {steps} "
                  f"steps of {len(picks)} group(s): seed phase {seed_ms:.3f} ms, whole selection "
                  f"{whole_ms:.1f} ms, {us:.2f} us per pick step = "
                  f"{step_mb / us:.2f} TB/s if every row were read (nearer {near})")
    # the torch loop: the global set, and one class of n / C rows
    for name, sub in ((("global", rows), (f"one class of {n // C} rows", rows[:n // C]))
                      if a.torch_steps else ()):
        seeds = torch.zeros(1, dtype=torch.int64, device=dev)
        ms = timed(lambda: torch_loop(sub, seeds, a.torch_steps))
        print(f"  torch loop, {name}: {ms * 1e3 / a.torch_steps:.1f} us per pick step over "
              f"{a.torch_steps} steps (difference, square-sum, minimum, argmax; no host sync)")


if __name__ == "__main__":
    main()
