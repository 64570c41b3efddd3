"""Rank process of the two-rank knn test (tests/test_gpu_knn_engine.py), started by
launch.launch_ranks:

    python knn_child.py OUT N

Every rank on cuda:0 in a gloo group (RCCL refuses two ranks on one device); each holds ONLY its
batch-aligned shard of the N synthetic examples and runs ScoringEngine.run(n_total=N) with EL2N,
nn and both knn scores over two checkpoints.  A row's neighbours may lie in the other shard: the
shard sizes and labels are all-gathered once per job and the feature rows once per checkpoint,
SHARED by nn and the knn scores, so a clean run makes K + 2 dist.all_gather calls for the scores
plus one per gathered score vector, which the child counts.  Rank 0 writes the gathered scores,
the keep-set and the call count to OUT (.npz); every rank checks its keep-set equals rank 0's.
"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

DATA_SEED, CKPT_SEEDS = 71, (14, 15)  # the test scores the same set in one process
METHODS = ("el2n", "nn", "knn", "knn_disagree")
MAX_GATHERS = len(CKPT_SEEDS) + 2 + len(METHODS)


def main(out, n):
    import numpy as np
    import torch
    import torch.distributed as dist
    from data_diet_distributed_amd import checkpoints, launch, synthetic
    from data_diet_distributed_amd.scoring import ScoreConfig, ScoringEngine, shard_bounds
    world, rank, _ = launch.rank_env()
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    launch.init_process_group("gloo", rank, world, timeout_s=300)
    calls = {"all_gather": 0}
    real = dist.all_gather

    def counted(*a, **k):
        calls["all_gather"] += 1
        return real(*a, **k)
    dist.all_gather = counted
    lo, hi = shard_bounds(n, 128, world, rank)
    images, labels = synthetic.make_images(n, 10, seed=DATA_SEED, lo=lo, hi=hi)
    sds = [synthetic.make_checkpoint("resnet18", 10, seed=s)["net"] for s in CKPT_SEEDS]
    models = checkpoints.build_models(sds, device=dev)
    img, lab = torch.from_numpy(images).to(dev), torch.from_numpy(labels).to(dev)
    eng = ScoringEngine(models, ScoreConfig(methods=METHODS, select_by="knn"), dev)
    full, kept, k = eng.run(img, lab, 0.5, n_total=n)
    n_calls = calls["all_gather"]
    dist.all_gather = real
    kept = kept.cpu()
    k0 = kept.clone()
    dist.broadcast(k0, 0)
    same = bool(torch.equal(kept, k0))
    if rank == 0:
        np.savez(out, kept=kept.numpy(), k=k, world=dist.get_world_size(),
                 backend=dist.get_backend(), shard=np.array([lo, hi]), all_gather=n_calls,
                 fallback=len(eng.fallback), **{m: full[m].cpu().numpy() for m in METHODS})
    dist.barrier()
    dist.destroy_process_group()
    print(f"RANK {rank} shard [{lo}, {hi}): keep-set equal to rank 0's: {same}; "
          f"{n_calls} all_gather call(s)", flush=True)
    return 0 if same and n_calls <= MAX_GATHERS else 1


if __name__ == "__main__":
    sys.exit(main(sys.argv[1], int(sys.argv[2])))
