"""Device-event times of one checkpoint's kmeans score beside proto and knn on the same rows
(profiles/kmeans/kernels_micro.txt):

    python tools/kmeans_micro.py [--n 50000] [--d 512] [--k 10] [--iters 20] [--reps 5] [--warm 2]

kmeans: the seed rows, `iters` Lloyd updates (dd_kmeans_assign with sums + dd_kmeans_centroids) and
the scoring assignment, as KMeansScore.end_checkpoint issues them on one rank.  proto: the sums,
the centroids and the distances, as ProtoScore.end_checkpoint.  knn: one dd_knn call, k = 5.
"""
import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from data_diet_distributed_amd import _capi, forward_scores  # noqa: E402


def timed(fn, warm, reps):
    for _ in range(warm):
        fn()
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(reps + 1)]
    ev[0].record()
    for i in range(reps):
        fn()
        ev[i + 1].record()
    torch.cuda.synchronize()
    return [ev[i].elapsed_time(ev[i + 1]) for i in range(reps)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=50000)
    ap.add_argument("--d", type=int, default=512)
    ap.add_argument("--k", type=int, default=10)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warm", type=int, default=2)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    n, D, k = a.n, a.d, a.k
    g = torch.Generator(device=dev).manual_seed(1)
    # ten planted classes on pooled post-ReLU-like rows
    lab = torch.randint(0, 10, (n,), generator=g, device=dev)
    centres = torch.randn((10, D), generator=g, device=dev)
    rows = (centres[lab] + torch.randn((n, D), generator=g, device=dev)).clamp_(min=0).add_(0.5)

    class Linear:
        out_features, in_features = 10, D

    class Cfg:
        batch_size = 128

    km = forward_scores.KMeansScore(lab, Linear, None, [n], 0, "f16x3", k, a.iters)
    proto = forward_scores.ProtoScore(lab, Linear, None, Cfg.batch_size)
    ids = torch.arange(n, dtype=torch.int64, device=dev)
    acc = torch.zeros((2, n), dtype=torch.float32, device=dev)
    state = {"ws": None}

    def knn():
        state["ws"] = _capi.knn(rows, ids, rows, ids, 5, q_label=lab, c_label=lab,
                                accum_dist=acc[0], accum_disagree=acc[1], workspace=state["ws"])

    def one_assign():
        _capi.kmeans_assign(rows, km.centroids, repack_rows=False, accum=km.accum,
                            workspace=km.workspace)

    def one_update():
        forward_scores.lloyd_step(rows, km.centroids, km.reduce, km.workspace, "f16x3", False)

    print(f"n={n} D={D}: kmeans k={k} iters={a.iters}; proto 10 classes; knn k=5")
    for name, fn in (("kmeans, one checkpoint", lambda: km.end_checkpoint(rows)),
                     ("  one Lloyd update (clear + assign with sums + centroids)", one_update),
                     ("  the scoring assignment alone", one_assign),
                     ("proto, one checkpoint", lambda: proto.end_checkpoint(rows)),
                     ("knn, one checkpoint", knn)):
        ms = timed(fn, a.warm, a.reps)
        print(f"  {name:58s} {np.mean(ms):9.3f} ms (min {min(ms):.3f}, max {max(ms):.3f})")
    counts = km.reduce[k * D:k * D + k].tolist()
    print(f"  cluster sizes after the last update: {counts}")


if __name__ == "__main__":
    main()
