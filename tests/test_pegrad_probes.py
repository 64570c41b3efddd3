"""The probe list of tests/helpers/pegrad_probes.py is sharp before a kernel is held to it: on
every launch's one-channel probes, each damaged variant of the kernel's arithmetic (a lo product
of the bf16 split dropped, both dropped, fp32 operands rounded to bf16) is at least 4 x outside
the bound tests/test_gpu_pegrad_probes.py applies to that launch.  CPU only."""
import numpy as np
import pytest

from data_diet_distributed_amd import _capi
from helpers import pegrad_probes as pp

SEPARATION = 4.0


@pytest.mark.parametrize("la", pp.LAUNCHES, ids=lambda la: la.name)
def test_damaged_variants_miss_the_bound(la):
    c = la.case()
    bar = pp.bound(la, c, c.pair)
    assert np.all(c.e3[c.zero] == 0)
    assert c.pair.sum() >= 2
    for name, sq in c.damaged.items():
        e = pp.err(sq[c.pair], c.ref[c.pair])
        print(f"SEP {la.name} {name} damaged={e:.3e} bound={bar:.3e} ratio={e / bar:.1f}")
        assert e >= SEPARATION * bar, (name, e, bar)


def test_names_are_unique():
    names = [la.name for la in pp.LAUNCHES]
    assert len(set(names)) == len(names)


def test_every_family_and_instance_is_listed():
    assert {la.family for la in pp.LAUNCHES} == set(pp.FAMILIES)
    assert {la.instance for la in pp.LAUNCHES} == set(pp.INSTANCES)
    for la in pp.LAUNCHES:  # a conv launch's name carries its instance's template arguments
        if "<" in la.instance and la.family not in ("linear", "bn"):
            assert la.instance[la.instance.index("<"):] in la.name, la.name


def test_persistent_kernels_have_handover_launches():
    """Each persistent instance has a one-step and a two-step launch with more tiles than
    workgroups, 130 outputs and column scales; at the full batch and at its first third every
    hand-over of a workgroup changes the tile's (c-block, o-block), and for each instance and
    step count some launch changes the o-block, and with it the column scales, at every one."""
    for inst in pp.PERSISTENT:
        las = [la for la in pp.LAUNCHES if la.instance == inst and la.handover]
        assert sorted(la.ho // 2 for la in las if la.cout == 130) == [1, 2], inst
        for steps in (1, 2):
            rotates = []
            for la in (la for la in las if la.ho // 2 == steps):
                B = la.case().B
                assert la.scale and B >= 200
                for n in (B, B // 3):
                    hand = la.handovers(n)
                    assert la.tiles(n) > pp.CUS and hand
                    assert all(a != b for a, b in hand), la.name
                rotates.append(all(a[1] != b[1] for n in (B, B // 3) for a, b in la.handovers(n)))
            assert any(rotates), (inst, steps)


@pytest.mark.parametrize("la", [la for la in pp.LAUNCHES if hasattr(la, "kernel")],
                         ids=lambda la: la.name)
def test_dispatch(la):
    """The launch resolves to the kernel family its name says (host logic of libdd.so)."""
    assert _capi.conv_method(la.geom(la.case().B), la.method, la.prec) == la.kernel
