"""Device-event times of dd_nn_same_class (profiles/nn/kernels_micro.txt):

    python tools/nn_micro.py [--reps 5] [--warm 2]

Every query of a class against every candidate of it, queries = candidates (the one-rank engine
call).  flop = 2 D sum_c n_c^2 (the algorithm's; the split MFMA does three times that).
"""
import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from data_diet_distributed_amd import _capi  # noqa: E402

# (class sizes, D, what)
SHAPES = (
    ((5000,) * 10, 512, "CIFAR-10 train set, ResNet-18 rows"),
    ((500,) * 100, 2048, "50 000 rows, 100 classes, ResNet-50 rows"),
    ((1281,) * 100, 2048, "100 ImageNet-sized classes, ResNet-50 rows"),
    ((150, 90, 60), 512, "tests/test_gpu_nn.py d512"),
    ((97, 203), 100, "tests/test_gpu_nn.py d100 (its largest class)"),
)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warm", type=int, default=2)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    for sizes, D, what in SHAPES:
        n, C = int(sum(sizes)), len(sizes)
        g = torch.Generator(device=dev).manual_seed(1)
        rows = torch.randn((n, D), generator=g, device=dev).clamp_(min=0).add_(0.5)
        ids = torch.arange(n, dtype=torch.int64, device=dev)
        off = torch.tensor(np.concatenate([[0], np.cumsum(sizes)]), dtype=torch.int64, device=dev)
        flop = 2.0 * D * sum(s * s for s in sizes)
        print(f"n={n} D={D} C={C} ({what}; {flop / 1e12:.3f} TFLOP, workspace "
              f"{_capi.nn_workspace_bytes(n, n, D) / 1e6:.0f} MB)")
        for operands in ("f16x3", "bf16x3"):
            acc = torch.zeros(n, dtype=torch.float32, device=dev)
            ws = None
            for _ in range(a.warm):
                ws = _capi.nn_same_class(rows, ids, off, rows, ids, off, operands=operands,
                                         accum=acc, workspace=ws)
            ev = [torch.cuda.Event(enable_timing=True) for _ in range(a.reps + 1)]
            ev[0].record()
            for i in range(a.reps):
                _capi.nn_same_class(rows, ids, off, rows, ids, off, operands=operands,
                                    accum=acc, workspace=ws)
                ev[i + 1].record()
            torch.cuda.synchronize()
            ms = [ev[i].elapsed_time(ev[i + 1]) for i in range(a.reps)]
            print(f"  {operands:7s}: {np.mean(ms):9.3f} ms per call (min {min(ms):.3f}, max "
                  f"{max(ms):.3f}; pack + search + value) = {flop / np.mean(ms) / 1e9:7.1f} "
                  f"TFLOP/s algorithmic")


if __name__ == "__main__":
    main()
