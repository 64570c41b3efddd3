"""The persistent 16-wide GraNd 3x3 norm kernel, 64 x 64 tile (DD_PEGRAD_WIDE=0) against the
64 c x 128 o workgroup (DD_PEGRAD_WIDE=1): the two arms alternating in one process, B = 1024,
the two ResNet-18 bench shapes; checks that both arms give the same bits.
  python tools/ab_pegrad_wide.py [alternations] [launches per timing]"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from data_diet_distributed_amd import _capi  # noqa: E402

SHAPES = {"128->128 16x16 s1": (128, 16, 128, 1), "64->128 32->16 s2": (64, 32, 128, 2)}


def main():
    dev = torch.device("cuda:0")
    alts = int(sys.argv[1]) if len(sys.argv) > 1 else 6
    iters = int(sys.argv[2]) if len(sys.argv) > 2 else 200
    B = 1024
    for name, (cin, H, cout, s) in SHAPES.items():
        g = torch.Generator(device=dev).manual_seed(0)
        act = torch.relu(torch.randn(B, cin, H, H, device=dev, generator=g))
        gout = torch.randn(B, cout, H // s, H // s, device=dev, generator=g) * 1e-2
        geom = _capi.conv_geom(act, gout, (3, 3), s, 1)
        ws = torch.empty(_capi.conv_workspace_bytes(geom, "direct", "bf16x3"),
                         dtype=torch.uint8, device=dev)

        def launch(sq, n):
            for _ in range(n):
                _capi.conv_pegrad_sqnorm(act, gout, (3, 3), s, 1, sq, ws, method="direct",
                                         precision="bf16x3")

        sq = torch.zeros(B, device=dev)
        launch(sq, 400)  # settle the clocks before the first arm
        torch.cuda.synchronize()
        res = {"0": [], "1": []}
        sqs = {}
        for _ in range(alts):
            for knob in ("0", "1"):
                os.environ["DD_PEGRAD_WIDE"] = knob  # read per call
                launch(sq, 10)
                torch.cuda.synchronize()
                e0 = torch.cuda.Event(enable_timing=True)
                e1 = torch.cuda.Event(enable_timing=True)
                e0.record()
                launch(sq, iters)
                e1.record()
                torch.cuda.synchronize()
                res[knob].append(e0.elapsed_time(e1) * 1e3 / iters)
                sqs[knob] = torch.zeros(B, device=dev)
                launch(sqs[knob], 1)
        assert torch.equal(sqs["0"], sqs["1"])
        for k in ("0", "1"):
            v = res[k]
            print(f"{name:22s} DD_PEGRAD_WIDE={k}: us/call (kernel + reduce) "
                  + " ".join(f"{x:7.1f}" for x in v)
                  + f"  mean {sum(v) / len(v):7.1f} spread {max(v) - min(v):5.1f}", flush=True)


if __name__ == "__main__":
    main()
