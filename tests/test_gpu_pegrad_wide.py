"""The 64 c x 128 o workgroup of the persistent 16-wide GraNd 3x3 norm kernel (DD_PEGRAD_WIDE=1)
writes bitwise the partials of the 64 x 64 tile (DD_PEGRAD_WIDE=0), and both meet the float64
oracle at the norm tolerance."""
import functools

import numpy as np
import pytest
import torch

from data_diet_distributed_amd import _capi
from oracle import pegrad as o_pegrad

pytestmark = pytest.mark.gpu

RTOL = 1e-3  # the norm tolerance of tests/test_gpu_kernels.py

# (B, cin, H, W, cout, stride, col_scale)
CASES = [
    (3, 64, 16, 16, 128, 1, False),    # one full wide tile per c-block
    (2, 17, 16, 16, 130, 1, False),    # ragged channels on both sides, odd n_oblk
    (2, 128, 10, 16, 256, 1, False),   # 5 steps, two wide tiles per c-block, tile hand-over
    (2, 64, 12, 16, 64, 1, False),     # cout below a wide tile: the 64 x 64 path either way
    (2, 40, 32, 32, 70, 2, False),     # the stride-2 head, ragged
    (2, 64, 32, 32, 128, 2, False),    # the stride-2 head, exact
    (3, 70, 8, 16, 200, 1, True),      # column scales, ragged, a second half part padding
    (2, 64, 32, 32, 128, 2, True),     # column scales on the stride-2 head
    (600, 128, 4, 16, 128, 1, False),  # more tiles than workgroups of a persistent grid
]


@functools.lru_cache(maxsize=None)
def _case(case):
    B, cin, H, W, cout, s, scaled = case
    rng = np.random.default_rng(1000 + CASES.index(case))
    act = np.maximum(rng.normal(size=(B, cin, H, W)), 0).astype(np.float32)
    gout = (rng.normal(size=(B, cout, H // s, W // s)) * 1e-2).astype(np.float32)
    scale = rng.uniform(0.2, 2.0, size=cout).astype(np.float32) if scaled else None
    ref = o_pegrad.conv_pegrad_sqnorm(act, gout, 3, 3, s, 1, col_scale=scale)
    ref.setflags(write=False)
    return act, gout, scale, ref


@pytest.mark.parametrize("case", CASES, ids=lambda c: "x".join(str(int(v)) for v in c))
def test_wide_tile_is_bitwise_the_narrow_tile(cuda, case, monkeypatch):
    act, gout, scale, ref = _case(case)
    s = case[5]
    a, g = torch.from_numpy(act).to(cuda), torch.from_numpy(gout).to(cuda)
    cs = torch.from_numpy(scale).to(cuda) if scale is not None else None
    geom = _capi.conv_geom(a, g, (3, 3), s, 1)
    assert _capi.conv_method(geom, "direct", "bf16x3") == "direct3x3"
    nbytes = _capi.conv_workspace_bytes(geom, "direct", "bf16x3")
    out = {}
    for knob in ("0", "1"):
        monkeypatch.setenv("DD_PEGRAD_WIDE", knob)
        # a poisoned workspace: a partial the kernel does not write shows in sq
        ws = torch.full((nbytes // 4,), float("nan"), device=cuda).view(torch.uint8)
        sq = torch.zeros(case[0], device=cuda)
        _capi.conv_pegrad_sqnorm(a, g, (3, 3), s, 1, sq, ws, method="direct", precision="bf16x3",
                                 col_scale=cs)
        out[knob] = sq
    torch.cuda.synchronize()
    err = {k: np.abs(v.cpu().numpy().astype(np.float64) / ref - 1).max() for k, v in out.items()}
    print(f"{case}: max rel err narrow {err['0']:.2e} wide {err['1']:.2e}")
    assert torch.equal(out["0"], out["1"])
    for knob in ("0", "1"):
        np.testing.assert_allclose(out[knob].cpu().numpy().astype(np.float64), ref, rtol=RTOL)
