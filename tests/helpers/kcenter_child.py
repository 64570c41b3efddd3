"""Rank process of the two-rank kcenter test (tests/test_gpu_kcenter_engine.py), started by
launch.launch_ranks:

    python kcenter_child.py OUT N POLICY

Every rank on cuda:0 in a gloo group (RCCL refuses two ranks on one device); each holds ONLY its
batch-aligned shard of the N synthetic examples and runs ScoringEngine.run(n_total=N) with EL2N
over two checkpoints and the kcenter fill.  The rows of checkpoint kcenter_ckpt are all-gathered
once and every rank runs the identical selection on them: no collective inside the loop.  Rank 0
writes the scores, the keep-set and the selection record to OUT (.npz); every rank checks its
keep-set equals rank 0's.
"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

DATA_SEED, CKPT_SEEDS = 83, (21, 22)  # the test scores the same set in one process
SEED_FRAC, SPARSITY = 0.1, 0.5


def config(policy):
    from data_diet_distributed_amd.scoring import ScoreConfig
    return ScoreConfig(methods=("el2n",), select_fill="kcenter", kcenter_seed_frac=SEED_FRAC,
                       select_policy=policy, kcenter_ckpt=0)


def main(out, n, policy):
    import numpy as np
    import torch
    import torch.distributed as dist
    from data_diet_distributed_amd import checkpoints, launch, synthetic
    from data_diet_distributed_amd.scoring import ScoringEngine, shard_bounds
    world, rank, _ = launch.rank_env()
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    launch.init_process_group("gloo", rank, world, timeout_s=300)
    lo, hi = shard_bounds(n, 128, world, rank)
    images, labels = synthetic.make_images(n, 10, seed=DATA_SEED, lo=lo, hi=hi)
    sds = [synthetic.make_checkpoint("resnet18", 10, seed=s)["net"] for s in CKPT_SEEDS]
    models = checkpoints.build_models(sds, device=dev)
    img, lab = torch.from_numpy(images).to(dev), torch.from_numpy(labels).to(dev)
    eng = ScoringEngine(models, config(policy), dev)
    full, kept, k = eng.run(img, lab, SPARSITY, n_total=n)
    kept = kept.cpu()
    k0 = kept.clone()
    dist.broadcast(k0, 0)
    same = bool(torch.equal(kept, k0))
    if rank == 0:
        np.savez(out, kept=kept.numpy(), k=k, world=dist.get_world_size(),
                 shard=np.array([lo, hi]), el2n=full["el2n"].cpu().numpy(),
                 radius=np.array(eng.last_selection["radius"]),
                 class_seeds=np.array(eng.last_selection["class_seeds"]))
    dist.barrier()
    dist.destroy_process_group()
    print(f"RANK {rank} shard [{lo}, {hi}): keep-set equal to rank 0's: {same}", flush=True)
    return 0 if same else 1


if __name__ == "__main__":
    sys.exit(main(sys.argv[1], int(sys.argv[2]), sys.argv[3]))
