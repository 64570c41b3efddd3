"""Device-event times of dd_knn (profiles/knn/kernels_micro.txt):

    python tools/knn_micro.py [--reps 5] [--warm 2]

Every query against every candidate of any class.  flop = 2 D nq nc (the algorithm's; the split
MFMA does three times that).  The yardstick is dd_nn_same_class at 50 000 x 512 in 10 classes
(tools/nn_micro.py): the same MFMA inner loop, a tenth of the flop, no list upkeep.
"""
import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from data_diet_distributed_amd import _capi  # noqa: E402

# (nq, nc, D, k, splits, what)
SHAPES = (
    (50000, 50000, 512, 1, 0, "CIFAR-10 train set, ResNet-18 rows, one rank"),
    (50000, 50000, 512, 5, 0, "the same, the default k"),
    (50000, 50000, 512, 16, 0, "the same, the largest k"),
    (50000, 50000, 512, 5, 1, "the same, k = 5, one segment"),
    (6250, 50000, 512, 5, 1, "a shard of eight ranks, one segment: 49 workgroups"),
    (6250, 50000, 512, 5, 0, "a shard of eight ranks, the automatic split count"),
    (50000, 50000, 2048, 5, 0, "50 000 ResNet-50 rows"),
    (300, 300, 512, 5, 0, "tests/test_gpu_knn.py d512"),
)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warm", type=int, default=2)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    for nq, nc, D, k, splits, what in SHAPES:
        g = torch.Generator(device=dev).manual_seed(1)
        cand = torch.randn((nc, D), generator=g, device=dev).clamp_(min=0).add_(0.5)
        rows = cand[:nq]
        q_id = torch.arange(nq, dtype=torch.int64, device=dev)
        c_id = torch.arange(nc, dtype=torch.int64, device=dev)
        lab = torch.randint(0, 10, (nc,), generator=g, device=dev)
        flop = 2.0 * D * nq * nc
        need = _capi.knn_workspace_bytes(nq, nc, D, k, splits)
        print(f"nq={nq} nc={nc} D={D} k={k} splits={splits} ({what}; {flop / 1e12:.3f} TFLOP, "
              f"workspace {need / 1e6:.0f} MB)")
        for operands in ("f16x3", "bf16x3"):
            acc = torch.zeros((2, nq), dtype=torch.float32, device=dev)
            kw = dict(q_label=lab[:nq], c_label=lab, splits=splits, operands=operands,
                      accum_dist=acc[0], accum_disagree=acc[1])
            ws = None
            for _ in range(a.warm):
                ws = _capi.knn(rows, q_id, cand, c_id, k, workspace=ws, **kw)
            ev = [torch.cuda.Event(enable_timing=True) for _ in range(a.reps + 1)]
            ev[0].record()
            for i in range(a.reps):
                _capi.knn(rows, q_id, cand, c_id, k, workspace=ws, **kw)
                ev[i + 1].record()
            torch.cuda.synchronize()
            ms = [ev[i].elapsed_time(ev[i + 1]) for i in range(a.reps)]
            print(f"  {operands:7s}: {np.mean(ms):9.3f} ms per call (min {min(ms):.3f}, max "
                  f"{max(ms):.3f}; pack + search + merge) = {flop / np.mean(ms) / 1e9:7.1f} "
                  f"TFLOP/s algorithmic")


if __name__ == "__main__":
    main()
