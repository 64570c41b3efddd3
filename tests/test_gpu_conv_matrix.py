"""Every tile x epilogue pair of the hand-written conv family (tests/helpers/conv_launches.py)
on its default path against a float64 reference of the same operation.

Float outputs: max-abs error over the reference's max-abs.
  bf16-halves launches: at most K_E3 x e3, e3 being the error of the float64 three-product
    emulation (bf16 hi/lo of both operands, hi.hi + hi.lo + lo.hi) on the same inputs.  K_E3 is
    1.5 x the largest kernel / emulation ratio measured over the whole list
    (profiles/conv_matrix/README.md) and may not exceed 4: 4 x e3 is where one lo half lost on
    one tap of one channel starts to show.
  fp16-halves launches: F16_REL of tests/test_gpu_f16_operands.py.
  the fused unit output x_out (fp32 element-wise ops, no split): 1e-6 as bn_apply's tests.
Statistics go through bn_finalize against float64 group statistics (2e-4 bf16, 2e-5 fp16, as
tests/test_gpu_el2n_fast.py and tests/test_gpu_f16_operands.py).  Fragment masks are checked
through a consumer and plane bits exactly (the launch's check()).

Two exact properties on the conv3x3 and down launches: example i of a B-example launch is
bitwise the one-example launch of x[i:i+1] (tiles hold up to 16 images), and scaling the
activations (or dy) of a plain bf16 launch by 2^-40 scales its output by exactly 2^-40.
"""
import pytest
import torch

from data_diet_distributed_amd import _capi
from helpers import conv_launches as cl

pytestmark = pytest.mark.gpu

K_E3 = 1.6  # 1.5 x 1.062, the largest of the 409 measured ratios (0.957 to 1.062)
assert K_E3 <= 4.0
F16_REL = 2e-6
XOUT_REL = 1e-6
STAT_REL = {"bf16x3": 2e-4, "f16x3": 2e-5}


def _rel(got, want):
    return ((got.double() - want).abs().max() / want.abs().max()).item()


def _close(got, want, rel):
    err = (got.detach().cpu().double() - want).abs().max().item()
    scale = want.abs().max().item()
    assert err <= rel * scale + 1e-6, (err, scale)


@pytest.mark.parametrize("la", cl.LAUNCHES, ids=lambda la: la.name)
def test_launch_against_float64(cuda, la):
    inp = la.inputs()
    out = la.run(inp, cuda)
    ref = la.ref(inp, out)
    for key, (want, emu) in ref.items():
        got = out[key].cpu()
        assert torch.isfinite(got).all(), f"{key}: an element was not written"
        err = _rel(got, want)
        if key == "x_out":
            bar = XOUT_REL
        elif la.operands == "f16x3":
            bar = F16_REL
        else:
            e3 = _rel(emu, want)
            bar = K_E3 * e3
            print(f"RATIO {la.name} {key} kernel={err:.3e} e3={e3:.3e} ratio={err / e3:.3f}")
        assert err <= bar, (key, err, bar)
    for st_key, y_key, gs, nst in la.stats:
        sc, sh = _capi.bn_finalize(out[st_key], inp["gamma"].to(cuda), inp["beta"].to(cuda),
                                   cl.EPS)
        rsc, rsh = cl.group_bn_ref(ref[y_key][0], gs, nst, inp["gamma"], inp["beta"])
        _close(sc, rsc, STAT_REL[la.operands])
        _close(sh, rsh, STAT_REL[la.operands])
    if la.check is not None:
        la.check(inp, out)


def test_unit_input_tiles(cuda):
    """The launch list's fused unit inputs are exactly the tiles the library offers them on."""
    assert tuple(t for t in cl.C3_TILES if cl.unit_input_supported(t)) == cl.C3_UNIT_TILES


def _floats(out):
    return {k: v for k, v in out.items() if not k.startswith("_") and v.is_floating_point()}


@pytest.mark.parametrize("la", [la for la in cl.LAUNCHES if la.slot is not None],
                         ids=lambda la: la.name)
def test_batch_slot(cuda, la):
    inp = la.inputs()
    full = _floats(la.run(inp, cuda))
    B = next(iter(full.values())).shape[0]
    for i in sorted({0, B // 2, B - 1}):
        one = _floats(la.run(la.slot(inp, i), cuda))
        for key, v in full.items():
            assert torch.equal(v[i:i + 1], one[key]), (key, i)


@pytest.mark.parametrize("la", [la for la in cl.LAUNCHES if la.scaled], ids=lambda la: la.name)
def test_power_of_two_scaling(cuda, la):
    inp = la.inputs()
    full = _floats(la.run(inp, cuda))
    small = dict(inp)
    for key in la.scaled:
        small[key] = inp[key] * cl.TWO_M40
    got = _floats(la.run(small, cuda))
    for key, v in full.items():
        assert (v != 0).any()
        assert torch.equal(got[key], v * cl.TWO_M40), key
