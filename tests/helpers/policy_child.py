"""Rank program of tests/test_gpu_select_policy.py (started by launch.launch_ranks as
`policy_child.py OUT`): every rank on cuda:0 in a gloo group, each holding ONLY its
batch-aligned shard of the 640 synthetic examples and of their labels, runs
ScoringEngine.run(n_total=640) with the stratified policy and a skip; the labels are gathered
for the selection.  Rank 0 writes the scores, the keep-set and the quotas to OUT (.npz); every
rank checks its keep-set equals rank 0's.  Not collected by pytest."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

N, C, DATA_SEED, CKPT_SEED = 640, 10, 83, 29  # tests/test_gpu_select_policy.py


def main(out):
    import numpy as np
    import torch
    import torch.distributed as dist

    from data_diet_distributed_amd import checkpoints, launch, synthetic
    from data_diet_distributed_amd.scoring import ScoreConfig, ScoringEngine, shard_bounds
    world, rank, _local = launch.rank_env()
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    launch.init_process_group("gloo", rank, world, timeout_s=120)
    lo, hi = shard_bounds(N, 128, world, rank)
    images, labels = synthetic.make_images(N, C, seed=DATA_SEED, lo=lo, hi=hi)
    sd = synthetic.make_checkpoint("resnet18", C, seed=CKPT_SEED)["net"]
    eng = ScoringEngine(checkpoints.build_models([sd], device=dev),
                        ScoreConfig(select_policy="stratified", select_skip=25), dev)
    full, kept, k = eng.run(torch.from_numpy(images).to(dev), torch.from_numpy(labels).to(dev),
                            0.5, n_total=N)
    kept = kept.cpu()
    k0 = kept.clone()
    dist.broadcast(k0, 0)
    same = bool(torch.equal(kept, k0))
    if rank == 0:
        np.savez(out, el2n=full["el2n"].cpu().numpy(), kept=kept.numpy(), k=k, world=world,
                 class_quota=np.array(eng.last_selection["class_quota"]),
                 class_skip=np.array(eng.last_selection["class_skip"]))
    dist.barrier()
    dist.destroy_process_group()
    print(f"RANK {rank} shard [{lo}, {hi}) keep-set equal to rank 0's: {same}", flush=True)
    return 0 if same else 1


if __name__ == "__main__":
    sys.exit(main(sys.argv[1]))
