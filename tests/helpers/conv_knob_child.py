"""Child process of tests/test_gpu_conv_knobs.py: runs one family's launches of
tests/helpers/conv_launches.py under the DD_* environment it was started with (the conv family
reads its once-per-process knobs at the first launch) and writes every output to an .npz:
"<launch>/<output>" -> the array's bytes, or their SHA-256 for outputs past 1 MiB.
Launches the library refuses under the setting (Launch.skip_env) are left out.  Prints
"child ok".  Not collected by pytest.

usage: conv_knob_child.py FAMILY OUT.npz"""
import hashlib
import os
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))                    # tests/
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))   # the repository root

DIGEST_OVER = 1 << 20  # bytes: larger outputs (the tile-count launches' tensors) as digests


def main(family, path):
    import numpy as np
    import torch

    from helpers import conv_launches as cl

    dev = torch.device("cuda:0")
    arrays = {}
    t0 = time.time()
    n = 0
    for la in cl.launches(family):
        if any(os.environ.get(k) == v for k, v in la.skip_env.items()):
            continue
        out = la.run(la.inputs(), dev)
        for key, t in out.items():
            if key.startswith("_"):
                continue
            raw = t.detach().cpu().contiguous().view(-1).view(torch.uint8).numpy()
            if raw.nbytes > DIGEST_OVER:
                raw = np.frombuffer(hashlib.sha256(raw.tobytes()).digest(), dtype=np.uint8)
            arrays[f"{la.name}/{key}"] = raw
        n += 1
    torch.cuda.synchronize()
    np.savez(path, **arrays)
    print(f"child ok {family} {n} launches {time.time() - t0:.2f} s")
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1], sys.argv[2]))
