"""The GraNd per-example norm kernels on the probes of tests/helpers/pegrad_probes.py: every
kernel instance dd_conv_pegrad_sqnorm can dispatch to, dd_linear_pegrad_sqnorm and
dd_bn_pegrad_sqnorm, each on one-channel, two-by-two, position, dense and zero probes (one per
example of the batch).

Precision: on each group of a launch's probes (pairs, position probes, 2x2 and dense) the max
  over examples of |sq / ref - 1| is at most K x the same figure of the float64 emulation of the
  kernel's stated arithmetic (e3) + 2^-20 (pegrad_probes.bound(); K is 1.5 x the largest
  measured kernel / e3 ratio, profiles/pegrad_probes/README.md).  A lo product lost on one tap,
  wave or channel is 19 x to 13000 x outside it (tests/test_pegrad_probes.py).
Exact properties, on every launch: a zero probe leaves sq bitwise alone; sq is added to;
  gout x 2^-12 and act x 2^5 scale sq by 2^-24 and 2^10 bitwise; an example's sq is bitwise the
  same with the batch reversed and cut to its first third (the persistent kernels with more
  tiles than workgroups, at both batch sizes, and a (c-block, o-block) that changes at every
  hand-over included; no kernel's summation order depends on B); with every buffer
  carved out of a NaN-filled one, sq is finite and inside the bound and no guard is written.
"""
import numpy as np
import pytest
import torch

from data_diet_distributed_amd import _capi
from helpers import pegrad_probes as pp

pytestmark = pytest.mark.gpu

GUARD = 1024  # floats on both sides of a carved buffer (4096 bytes: carve offsets stay aligned)
NAN_BITS = torch.tensor(float("nan")).view(torch.int32).item()

_BASE = {}


@pytest.fixture(params=pp.LAUNCHES, ids=lambda la: la.name)
def la(request, monkeypatch):
    for knob, value in request.param.env.items():
        monkeypatch.setenv(knob, value)  # read per call
    return request.param


def _to(inp, dev):
    return {k: v.to(dev) for k, v in inp.items()}


def _workspace(la, B, dev):
    # poisoned: a partial the kernel does not write shows in sq
    return torch.full((la.workspace_bytes(B) // 4,), float("nan"), device=dev).view(torch.uint8)


def _run(la, t, sq0=None):
    x = t[la.batched[0]]
    sq = torch.zeros(x.shape[0], device=x.device) if sq0 is None else sq0.clone()
    la.launch(t, sq, _workspace(la, x.shape[0], x.device))
    return sq


def _base(la, dev):
    """sq of the launch's own inputs from a zero start (computed once per launch)"""
    if la.name not in _BASE:
        _BASE[la.name] = _run(la, _to(la.case().inp, dev))
    return _BASE[la.name]


def _inside(la, c, got, extra=0.0, show=False):
    """every group of probes inside its own bound"""
    assert np.isfinite(got).all()
    for name, m in c.groups.items():
        e, e3, bar = pp.err(got[m], c.ref[m]), pp.err(c.e3[m], c.ref[m]), pp.bound(la, c, m)
        if show:
            print(f"RATIO {la.name} {la.arith} {name} kernel={e:.3e} e3={e3:.3e} "
                  f"ratio={e / e3:.3f}")
        assert e <= bar + extra, (name, e, e3, bar)


def test_precision(cuda, la):
    c = la.case()
    if hasattr(la, "kernel"):
        assert _capi.conv_method(la.geom(c.B), la.method, la.prec) == la.kernel
    got = _base(la, cuda).cpu().double().numpy()
    assert np.all(got[c.zero] == 0.0)
    _inside(la, c, got, show=True)


def test_accumulates_and_zero_probes_add_nothing(cuda, la):
    """sq starts at half the norm (0.75 on the zero probes).  fl(sq0 + s) is within 2^-24 of
    sq0 + s <= 1.5 s: at most 2^-23 of s on top of the bound."""
    c = la.case()
    sq0 = torch.from_numpy(np.where(c.zero, 0.75, 0.5 * c.ref)).float().to(cuda)
    sq = _run(la, _to(c.inp, cuda), sq0)
    zero = torch.from_numpy(c.zero).to(cuda)
    assert torch.equal(sq[zero], sq0[zero])
    got = (sq.double() - sq0.double()).cpu().numpy()
    _inside(la, c, got, 2.0 ** -23)


def test_power_of_two_homogeneity(cuda, la):
    """(magnitudes: pegrad_probes.Conv.homog)"""
    c = la.case()
    base = _base(la, cuda)
    assert (base != 0).any()
    for key, (e_in, e_out) in la.homog.items():
        t = _to(c.inp, cuda)
        t[key] = t[key] * 2.0 ** e_in
        assert torch.equal(_run(la, t), base * 2.0 ** e_out), key


def test_batch_slot_independence(cuda, la):
    c = la.case()
    base = _base(la, cuda)
    t = _to(c.inp, cuda)
    rev = {k: v.flip(0) if k in la.batched else v for k, v in t.items()}
    assert torch.equal(_run(la, rev).flip(0), base)
    n = c.B // 3
    cut = {k: v[:n].contiguous() if k in la.batched else v for k, v in t.items()}
    assert torch.equal(_run(la, cut), base[:n])


def _carve(x, dev, numel=None):
    """x (or numel poisoned floats) inside a NaN-filled device buffer: (buffer, view)"""
    n = x.numel() if numel is None else numel
    big = torch.full((2 * GUARD + n,), float("nan"), device=dev)
    view = big[GUARD:GUARD + n]
    if numel is None:
        view = view.view(x.shape)
        view.copy_(x)
    return big, view


def _guards_untouched(big):
    bits = big.view(torch.int32)
    return bool((bits[:GUARD] == NAN_BITS).all() and (bits[-GUARD:] == NAN_BITS).all())


def test_guard_bands(cuda, la):
    """act, gout, col_scale (v, g, r, gamma, beta), sq and the workspace carved out of NaN: a
    read past a ragged tail that reaches arithmetic, or a write past a buffer, shows."""
    c = la.case()
    bufs, t = {}, {}
    for k, v in c.inp.items():
        bufs[k], t[k] = _carve(v, cuda)
    bufs["sq"], sq = _carve(None, cuda, c.B)
    sq.zero_()
    nbytes = la.workspace_bytes(c.B)
    bufs["ws"], ws = _carve(None, cuda, nbytes // 4)
    ws = ws.view(torch.uint8)
    assert ws.numel() == nbytes
    la.launch(t, sq, ws)
    got = sq.cpu().double().numpy()
    assert np.all(got[c.zero] == 0.0)
    _inside(la, c, got)
    for k, big in bufs.items():
        assert _guards_untouched(big), k
    for k, v in c.inp.items():  # inputs are read only
        assert torch.equal(t[k].cpu(), v), k
