"""Device-event times of dd_kde, beside dd_knn (k = 10) at the same shapes in the same session
(DESIGN §4.15 records them):

    python tools/kde_micro.py [--reps 5] [--warm 2]

Every query against every candidate of any class.  flop = 2 D nq nc (the algorithm's; the split
MFMA does three times that).  The yardstick is dd_knn: the same pack and the same key scan, a
sorted-list insert where dd_kde has one exp2 per key (up to two where the labels are compared).
A call without candidates times the queries' pack, an empty fold and the merge; the kernels one
by one (pack, fold, merge) come from a kernel trace of `--only 0`.
"""
import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from data_diet_distributed_amd import _capi  # noqa: E402

# (nq, nc, D, seg_rows, what)
SHAPES = (
    (50000, 50000, 512, 0, "CIFAR-10 train set, ResNet-18 rows, one rank"),
    (50000, 50000, 512, 50048, "the same, one segment"),
    (6250, 50000, 512, 0, "a shard of eight ranks, the default segments"),
    (50000, 50000, 2048, 0, "50 000 ResNet-50 rows"),
    (300, 300, 512, 0, "tests/test_gpu_kde.py d512"),
)


def timed(fn, warm, reps):
    for _ in range(warm):
        fn()
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(reps + 1)]
    ev[0].record()
    for i in range(reps):
        fn()
        ev[i + 1].record()
    torch.cuda.synchronize()
    ms = [ev[i].elapsed_time(ev[i + 1]) for i in range(reps)]
    return np.mean(ms), min(ms), max(ms)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warm", type=int, default=2)
    ap.add_argument("--only", type=int, default=None, help="index of the one shape to run")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    for nq, nc, D, seg_rows, what in SHAPES if a.only is None else SHAPES[a.only:a.only + 1]:
        g = torch.Generator(device=dev).manual_seed(1)
        cand = torch.randn((nc, D), generator=g, device=dev).clamp_(min=0).add_(0.5)
        rows = cand[:nq]
        q_id = torch.arange(nq, dtype=torch.int64, device=dev)
        c_id = torch.arange(nc, dtype=torch.int64, device=dev)
        lab = torch.randint(0, 10, (nc,), generator=g, device=dev)
        inv = 1.0 / (0.25 * 2.0 * D * 0.34)  # tau = 0.25 on these rows' mean squared distance
        flop = 2.0 * D * nq * nc
        need = _capi.kde_workspace_bytes(nq, nc, D, seg_rows)
        print(f"nq={nq} nc={nc} D={D} seg_rows={seg_rows} ({what}; {flop / 1e12:.3f} TFLOP, "
              f"workspace {need / 1e6:.0f} MB)")
        acc = torch.zeros((2, nq), dtype=torch.float32, device=dev)
        ws = torch.empty(need, dtype=torch.uint8, device=dev)
        lab_kw = dict(q_label=lab[:nq], c_label=lab)
        knn_ws = torch.empty(_capi.knn_workspace_bytes(nq, nc, D, 10), dtype=torch.uint8,
                             device=dev)
        for operands in ("f16x3", "bf16x3"):
            runs = (
                ("kde, both scores", lambda: _capi.kde(
                    rows, q_id, cand, c_id, inv, seg_rows=seg_rows, operands=operands,
                    accum_nll=acc[0], accum_post=acc[1], workspace=ws, **lab_kw)),
                ("kde alone (no labels)", lambda: _capi.kde(
                    rows, q_id, cand, c_id, inv, seg_rows=seg_rows, operands=operands,
                    accum_nll=acc[0], workspace=ws)),
                ("pack + merge (no candidate)", lambda: _capi.kde(
                    rows, q_id, cand[:0], c_id[:0], inv, seg_rows=seg_rows, operands=operands,
                    accum_nll=acc[0], workspace=ws)),
                ("knn k = 10, both scores", lambda: _capi.knn(
                    rows, q_id, cand, c_id, 10, operands=operands, accum_dist=acc[0],
                    accum_disagree=acc[1], workspace=knn_ws, **lab_kw)),
            )
            for name, fn in runs:
                mean, lo, hi = timed(fn, a.warm, a.reps)
                print(f"  {operands:7s} {name:28s}: {mean:9.3f} ms per call (min {lo:.3f}, max "
                      f"{hi:.3f}) = {flop / mean / 1e9:7.1f} TFLOP/s algorithmic")


if __name__ == "__main__":
    main()
