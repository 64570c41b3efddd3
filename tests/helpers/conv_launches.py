"""One list of named launches of the hand-written conv family (dd_conv3x3_forward and its unit
input, dd_down_forward / dd_down_backward, dd_conv1x1_forward / dd_conv_gemm_forward) for
tests/test_gpu_conv_matrix.py (float64 references, in-process) and tests/test_gpu_conv_knobs.py
(bitwise against the same list run in a child process under another DD_* setting).  Data and
small functions only.

A Launch has
  name, family ("conv3x3" | "down" | "c1x1"), operands ("bf16x3" | "f16x3")
  inputs()         CPU tensors from a torch.Generator seeded by a stable hash of the name
  run(inp, dev)    the launch through _capi: {output name: device tensor}; "_..." keys carry
                   the BNStats objects and are not outputs
  ref(inp, out)    {output name: (float64 reference, float64 three-product emulation or None)}
  stats            [(BNStats key, output key, group size, n_stat)] checked through bn_finalize
  check(inp, out)  exact properties of the outputs (plane bits, mask_in == mask_src), or None
  slot(inp, i)     the one-example launch of example i (batch-slot property), or None
  scaled           input keys whose 2^-40 scaling must scale the output exactly, or None
  skip_env         {knob: value} under which the library refuses the launch
  big              a tile-count launch (large batch, plain inputs only)
  epi_stats        the *_EPI knob that swaps this statistics launch's kernel for one whose sums of
                   squares round differently (tests/test_gpu_conv_knobs.py), or None

Every buffer _capi allocates for a launch comes back poisoned (poisoned(): NaN, 0xFF bytes for
mask words and plane bits) and every statistics buffer zeroed, so an element a kernel should
have written and did not shows in both test modules.

The three-product emulation (emu3) is the arithmetic the bf16-halves kernels implement: both
operands split into bf16 hi + lo (round to nearest even, lo = bf16(v - hi)), the products
hi.hi + hi.lo + lo.hi summed exactly (float64).  Its distance from the float64 reference is the
error floor of the format; the kernels add fp32 accumulation on top.
"""
import contextlib
import hashlib
import math

import torch
import torch.nn.functional as F

from data_diet_distributed_amd import _capi

FAMILIES = ("conv3x3", "down", "c1x1")
EPS = 1e-5
TWO_M40 = 2.0 ** -40


def seed_of(name: str) -> int:
    return int.from_bytes(hashlib.sha256(name.encode()).digest()[:8], "little") >> 1


class Launch:
    def __init__(self, name, family, operands, build, run, ref, stats=(), check=None, slot=None,
                 scaled=None, skip_env=None, big=False, epi_stats=None):
        self.name, self.family, self.operands = name, family, operands
        self._build, self.run, self.ref = build, run, ref
        self.stats, self.check, self.slot, self.scaled = list(stats), check, slot, scaled
        self.skip_env, self.big, self.epi_stats = dict(skip_env or {}), big, epi_stats

    def inputs(self):
        return self._build(torch.Generator().manual_seed(seed_of(self.name)))

    def __repr__(self):
        return self.name


# ---- poisoned allocations --------------------------------------------------------------------
class _PoisonTorch:
    """torch, with empty / empty_like returning poisoned memory."""

    def __getattr__(self, name):
        return getattr(torch, name)

    @staticmethod
    def _fill(t):
        if t.numel():
            if t.is_floating_point():
                t.fill_(float("nan"))
            else:
                t.view(torch.uint8).fill_(255)
        return t

    def empty(self, *a, **k):
        return self._fill(torch.empty(*a, **k))

    def empty_like(self, *a, **k):
        return self._fill(torch.empty_like(*a, **k))


def _zero_stats(buf, G, C, tiles, device):
    # (zeroed: the slots of a ragged last group past B are never written)
    return torch.zeros(G * C * tiles * 2, dtype=torch.float32, device=device)


@contextlib.contextmanager
def poisoned():
    saved = _capi.torch, _capi._stats_buffer
    _capi.torch, _capi._stats_buffer = _PoisonTorch(), _zero_stats
    try:
        yield
    finally:
        _capi.torch, _capi._stats_buffer = saved


# ---- float64 references ----------------------------------------------------------------------
def _split(t):
    t = t.float()
    hi = t.bfloat16().float()
    lo = (t - hi).bfloat16().float()
    return hi.double(), lo.double()


def emu3(lin, x, w):
    """lin(x, w) (bilinear) in the three split products of bf16 halves, summed in float64; x is
    rounded to fp32 first (the staged value the kernel splits)."""
    xh, xl = _split(x)
    wh, wl = _split(w)
    return lin(xh, wh) + lin(xh, wl) + lin(xl, wh)


def ex(t, gs, B):
    """[G, C] per-group rows -> [B, C, 1, 1] per-example, float64."""
    return t.double().repeat_interleave(gs, 0)[:B, :, None, None]


def group_gs(B, e=1):
    """The smallest group size (a multiple of e images per tile) whose last group is ragged and
    still holds an example below n_stat = B - 1."""
    m = e
    while B % m == 0 or B - 1 <= (-(-B // m) - 1) * m:
        m += e
    return m


def group_bn_ref(y, gs, n_valid, gamma, beta):
    """Per-group train-mode BN affine (scale, shift) of y (float64) over rows < n_valid."""
    B, C = y.shape[:2]
    G = -(-B // gs)
    sc = torch.zeros(G, C, dtype=torch.float64)
    sh = torch.zeros(G, C, dtype=torch.float64)
    for g in range(G):
        lo, hi = g * gs, min(B, (g + 1) * gs, n_valid)
        assert hi > lo, "the launch list keeps every group non-empty"
        v = y[lo:hi].double()
        mean = v.mean(dim=(0, 2, 3))
        var = v.var(dim=(0, 2, 3), unbiased=False)
        sc[g] = gamma.double() / torch.sqrt(var + EPS)
        sh[g] = beta.double() - mean * sc[g]
    return sc, sh


def plane_bits(pos):
    """(bool tensor, numel % 32 == 0) -> int32 plane words, bit p & 31 of word p >> 5."""
    v = (pos.reshape(-1, 32).to(torch.int64) << torch.arange(32)).sum(1)
    return (v - ((v >> 31) << 32)).to(torch.int32)


def _both(lin, x, w, epi, bf16):
    return epi(lin(x, w.double())), (epi(emu3(lin, x, w)) if bf16 else None)


def _sliced(inp, i, keys):
    out = dict(inp)
    for k in keys:
        out[k] = inp[k][i:i + 1].contiguous()
    return out


# ---- conv3x3 ---------------------------------------------------------------------------------
# epilogue sets: b bias, r ReLU, R residual, s mask_src, o mask_out, i mask_in, S statistics,
# a staging transform (in_affine)
C3_EPI = {"plain": "", "stats": "S", "stats_aff": "Sa", "fwd": "bro", "fwdres": "broR",
          "bwd": "i", "bwdres": "iR", "msrc": "s", "brr": "bRr", "resmsrc": "Rs", "aff": "a"}
# dispatch_epi_t has an fp16 instance of every epilogue (the generic one where none is specialised)
C3_F16 = tuple(e for e in C3_EPI if e != "aff")
# a tile reached only by a grouped launch gets every epilogue with the staging transform.  Its
# fragment masks are written and read by the kernel in its own tile's order, in a buffer sized
# by the ungrouped geometry of the shape (dd_conv3x3_mask_bytes: another tile's, never smaller),
# so a grouped producer and a grouped consumer agree; plane bits do not exist at 4x4
C3_GROUPED = {"aff": "a", "stats": "S", "stats_aff": "Sa", "fwd": "broa", "fwdres": "broRa",
              "bwd": "ia", "bwdres": "iRa", "brr": "bRra", "msrc": "sa", "resmsrc": "Rsa"}

# tile: (shape (B, cin, cout, H, W), images per tile, grouped-only)
C3_TILES = {
    "narrow32": ((2, 20, 70, 8, 32), 1, False),
    "r2w16": ((2, 20, 70, 8, 16), 1, False),
    "narrow16": ((2, 20, 40, 8, 16), 1, False),
    "r2w8": ((3, 20, 70, 8, 8), 2, False),
    "narrow8e2": ((3, 20, 40, 8, 8), 2, False),
    "narrow8e1": ((2, 20, 40, 16, 8), 1, False),
    "r2w4": ((11, 20, 70, 4, 4), 8, False),
    "wide4": ((19, 20, 40, 4, 4), 16, False),
    "narrow4": ((6, 20, 70, 4, 4), 4, True),
    "stem32": ((2, 3, 64, 8, 32), 1, False),
    "stem16": ((2, 3, 128, 8, 16), 1, False),
}
# a batch that makes two groups under group_gs (r2w4, wide4 and narrow4 have two already)
C3_TWO_GROUPS = {"narrow32": 5, "r2w16": 5, "narrow16": 5, "r2w8": 7, "narrow8e2": 7,
                 "narrow8e1": 5, "stem32": 5, "stem16": 5}
# the tiles whose fused unit input exists (conv3x3_unit_input_supported says so for exactly
# these: test_gpu_conv_matrix.py::test_unit_input_tiles)
C3_UNIT_TILES = ("narrow32", "r2w16", "r2w8")
# tile-count launches (plain): more tiles than two per CU of a 256-CU device, and 13 tiles
C3_COUNTS = {
    "narrow32": [(70, 20, 40, 32, 32), (13, 20, 40, 4, 32)],
    "r2w16": [(264, 20, 70, 16, 16), (13, 20, 70, 8, 16)],
    "narrow16": [(264, 20, 40, 16, 16), (13, 20, 40, 8, 16)],
    "r2w8": [(1042, 20, 70, 8, 8), (25, 20, 70, 8, 8)],
    "narrow8e2": [(1042, 20, 40, 8, 8), (25, 20, 40, 8, 8)],
    "narrow8e1": [(261, 20, 40, 16, 8), (1, 20, 40, 104, 8)],
    "r2w4": [(2100, 20, 70, 4, 4), (4104, 20, 70, 4, 4), (101, 20, 70, 4, 4)],
    "wide4": [(8200, 20, 40, 4, 4), (205, 20, 40, 4, 4)],
    "narrow4": [(1048, 20, 70, 4, 4), (50, 20, 40, 4, 4)],
}


def _c3(tile, shape, e, grouped_only, epi, ops, big=False):
    B, cin, cout, H, W = shape
    fl = (C3_GROUPED if grouped_only else C3_EPI)[epi]
    has = lambda c: c in fl  # noqa: E731
    grouped = has("S") or has("a")
    gs = (4 if grouped_only else group_gs(B, e)) if grouped else None
    G = -(-B // gs) if grouped else 1
    nst = B - 1
    bf16 = ops == "bf16x3"
    name = f"c3-{tile}-{'x'.join(map(str, shape))}-{epi}-{ops}"
    bits_ok = has("o") and (H * W) % 32 == 0

    def build(g):
        d = {"x": torch.randn(B, cin, H, W, generator=g),
             "w": torch.randn(cout, cin, 3, 3, generator=g) / (3 * cin ** 0.5),
             "sc": torch.rand(G, cin, generator=g) + 0.5,
             "sh": torch.randn(G, cin, generator=g) * 0.3}
        if big:
            return d
        d.update(bias=torch.randn(cout, generator=g), res=torch.randn(B, cout, H, W, generator=g),
                 msk=torch.randn(B, cout, H, W, generator=g),
                 gamma=torch.rand(cout, generator=g) + 0.5, beta=torch.randn(cout, generator=g),
                 xp=torch.randn(B, cin, H, W, generator=g), bp=torch.randn(cout, generator=g))
        return d

    def run(inp, dev):
        t = lambda k: inp[k].to(dev)  # noqa: E731
        out = {}
        with poisoned():
            pk = _capi.conv3x3_pack(t("w"), operands=ops)
            kw = {}
            if has("b"):
                kw["bias"] = t("bias")
            if has("r"):
                kw["relu"] = True
            if has("R"):
                kw["residual"] = t("res")
            if has("s"):
                kw["mask_src"] = t("msk")
            if has("a"):
                kw.update(in_affine=(t("sc"), t("sh")), group_size=gs)
            if has("S"):
                kw.update(stats=True, group_size=gs, n_stat=nst)
            if has("o"):
                kw["mask_out"] = out["mask"] = _capi.conv3x3_mask(B, cout, H, W, dev)
            if has("i"):
                # the producer of the fragment mask: a forward launch of the same geometry (the
                # same group, so the same tile), bias + ReLU, with the residual where the
                # consumer has one (the two specialised forward epilogues)
                same = {k: v for k, v in kw.items() if k in ("residual", "in_affine", "group_size")}
                mp = _capi.conv3x3_mask(B, cout, H, W, dev)
                out["h"] = _capi.conv3x3(t("xp"), pk, cout, bias=t("bp"), relu=True, mask_out=mp,
                                         **same)
                out["mask_p"] = mp
                out["y_src"] = _capi.conv3x3(t("x"), pk, cout, mask_src=out["h"], **same)
                kw["mask_in"] = mp
            y = _capi.conv3x3(t("x"), pk, cout, **kw)
            if has("S"):
                y, st = y
                out["stats"], out["_st"] = st.buf, st
            out["y"] = y
            if bits_ok:
                out["bits"] = _capi.conv3x3_mask_plane_bits(out["mask"], B, cout, H, W)
        return out

    def ref(inp, out):
        x = inp["x"].double()
        if has("a"):
            x = torch.relu(x * ex(inp["sc"], gs, B) + ex(inp["sh"], gs, B))

        def epi(z):
            if has("b"):
                z = z + inp["bias"].double()[None, :, None, None]
            if has("R"):
                z = z + inp["res"].double()
            if has("r"):
                z = torch.relu(z)
            if has("s"):
                z = z * (inp["msk"] > 0)
            if has("i"):
                z = z * (out["h"].cpu() > 0)
            return z
        return {"y": _both(lambda a, b: F.conv2d(a, b, padding=1), x, inp["w"], epi, bf16)}

    def check(inp, out):
        if bits_ok:
            assert torch.equal(out["bits"].cpu(), plane_bits(out["y"].cpu() > 0)), "plane bits"
        if has("o"):
            assert (out["y"] > 0).any() and (out["y"] == 0).any()
        if has("i"):
            assert torch.equal(out["y"], out["y_src"]), "mask_in != mask_src of the producer"

    free = not grouped and not has("i") and not big
    return Launch(name, "conv3x3", ops, build, run, ref,
                  stats=[("_st", "y", gs, nst)] if has("S") else (),
                  check=check if (has("o") or has("i")) else None,
                  slot=(lambda inp, i: _sliced(inp, i, ("x", "res", "msk"))) if free else None,
                  scaled=("x",) if epi == "plain" and bf16 and not big else None, big=big)


def _c3_unit(tile, shape, mode, ops):
    B, cin, cout, H, W = shape
    gs, nst = group_gs(B, C3_TILES[tile][1]), B - 1
    G = -(-B // gs)
    bf16 = ops == "bf16x3"

    def build(g):
        r = lambda *s: torch.randn(*s, generator=g)  # noqa: E731
        return {"yp": r(B, cin, H, W), "res": r(B, cin, H, W),
                "sc": torch.rand(G, cin, generator=g) + 0.5, "sh": r(G, cin) * 0.3,
                "rsc": torch.rand(G, cin, generator=g) + 0.5, "rsh": r(G, cin) * 0.3,
                "w": r(cout, cin, 3, 3) / (3 * cin ** 0.5),
                "gamma": torch.rand(cout, generator=g) + 0.5, "beta": r(cout)}

    def run(inp, dev):
        t = lambda k: inp[k].to(dev)  # noqa: E731
        with poisoned():
            pk = _capi.conv3x3_pack(t("w"), operands=ops)
            xo, y, st = _capi.conv3x3_unit_input(
                t("yp"), (t("sc"), t("sh")), pk, cout, gs, n_stat=nst,
                residual=t("res") if mode != "none" else None,
                res_affine=(t("rsc"), t("rsh")) if mode == "affine" else None)
        return {"x_out": xo, "y": y, "stats": st.buf, "_st": st}

    def ref(inp, out):
        x = inp["yp"].double() * ex(inp["sc"], gs, B) + ex(inp["sh"], gs, B)
        if mode == "raw":
            x = x + inp["res"].double()
        elif mode == "affine":
            x = x + inp["res"].double() * ex(inp["rsc"], gs, B) + ex(inp["rsh"], gs, B)
        x = torch.relu(x)
        lin = lambda a, b: F.conv2d(a, b, padding=1)  # noqa: E731
        return {"x_out": (x, None), "y": _both(lin, x, inp["w"], lambda z: z, bf16)}

    return Launch(f"c3u-{tile}-{'x'.join(map(str, shape))}-{mode}-{ops}", "conv3x3", ops, build,
                  run, ref, stats=[("_st", "y", gs, nst)])


def _conv3x3_launches():
    out = []
    for tile, (shape, e, grouped_only) in C3_TILES.items():
        epis = C3_GROUPED if grouped_only else C3_EPI
        for epi in epis:
            if epi == "aff" and not grouped_only:
                continue
            out.append(_c3(tile, shape, e, grouped_only, epi, "bf16x3"))
            if epi in C3_F16 or grouped_only:
                out.append(_c3(tile, shape, e, grouped_only, epi, "f16x3"))
        # two groups (the issue's batches give one on most tiles): per-group affine rows and
        # statistics slots
        B2 = C3_TWO_GROUPS.get(tile)
        if B2:
            out.append(_c3(tile, (B2,) + shape[1:], e, grouped_only, "stats_aff", "bf16x3"))
        if tile in C3_UNIT_TILES:
            for mode in ("none", "raw", "affine"):
                for ops in ("bf16x3", "f16x3"):
                    out.append(_c3_unit(tile, shape, mode, ops))
            out.append(_c3_unit(tile, (B2,) + shape[1:], "affine", "bf16x3"))
    for tile, shapes in C3_COUNTS.items():
        _, e, grouped_only = C3_TILES[tile]
        for shape in shapes:
            out.append(_c3(tile, shape, e, grouped_only, "aff" if grouped_only else "plain",
                           "bf16x3", big=True))
    return out


def unit_input_supported(tile):
    (B, cin, cout, H, W), e, _ = C3_TILES[tile]
    return _capi.conv3x3_unit_input_supported(H, W, cin, cout, group_gs(B, e))


# ---- downsampling head -----------------------------------------------------------------------
DOWN_OUT = [(2, 32), (8, 16), (4, 16), (8, 8), (4, 4)]
DOWN_B, DOWN_CIN = 3, 20
DOWN_FLAGS = ("stats", "grand", "mixed", "plain")
DOWN_MANY = 530


def _down_gs(ho, wo, B=DOWN_B):
    return group_gs(B, 4 if (ho, wo) == (4, 4) else 1)


def _dn(ho, wo, cout, sc, flags, ops, B=DOWN_B):
    cin = DOWN_CIN
    gs, nst = _down_gs(ho, wo, B), B - 1
    bf16 = ops == "bf16x3"

    def build(g):
        r = lambda *s: torch.randn(*s, generator=g)  # noqa: E731
        return {"x": r(B, cin, 2 * ho, 2 * wo), "w3": r(cout, cin, 3, 3) / (3 * cin ** 0.5),
                "w1": r(cout, cin, 1, 1) / cin ** 0.5, "b3": r(cout), "b1": r(cout),
                "gamma": torch.rand(cout, generator=g) + 0.5, "beta": r(cout)}

    def run(inp, dev):
        t = lambda k: inp[k].to(dev)  # noqa: E731
        kw = {}
        if flags == "stats":
            kw = dict(group_size=gs, stats=True, n_stat=nst)
        elif flags in ("grand", "mixed"):
            kw = dict(bias=t("b3"), relu=True)
            if flags == "grand" and sc:
                kw["bias_sc"] = t("b1")
        with poisoned():
            p3 = _capi.conv3x3_pack(t("w3"), operands=ops)
            p1 = _capi.conv1x1_pack(t("w1"), operands=ops) if sc else None
            y, ys, st, sts = _capi.conv_down(t("x"), p3, cout, p1, **kw)
        out = {"y": y}
        if sc:
            out["y_sc"] = ys
        if st is not None:
            out["stats"], out["_st"] = st.buf, st
        if sts is not None:
            out["stats_sc"], out["_sts"] = sts.buf, sts
        return out

    def ref(inp, out):
        x = inp["x"].double()
        biased = flags in ("grand", "mixed")
        b3 = inp["b3"].double()[None, :, None, None]
        b1 = inp["b1"].double()[None, :, None, None]
        res = {"y": _both(lambda a, b: F.conv2d(a, b, stride=2, padding=1), x, inp["w3"],
                          (lambda z: torch.relu(z + b3)) if biased else (lambda z: z), bf16)}
        if sc:
            res["y_sc"] = _both(lambda a, b: F.conv2d(a, b, stride=2), x, inp["w1"],
                                (lambda z: z + b1) if flags == "grand" else (lambda z: z), bf16)
        return res

    stats = []
    if flags == "stats":
        stats = [("_st", "y", gs, nst)] + ([("_sts", "y_sc", gs, nst)] if sc else [])
    tag = "" if B == DOWN_B else f"-b{B}"
    return Launch(f"dn-{ho}x{wo}-c{cout}-{'sc' if sc else 'nosc'}-{flags}-{ops}{tag}", "down", ops,
                  build, run, ref, stats=stats, big=B > 64,
                  # fwd_epi: the shortcut-fused statistics launch is the EL2N flag set
                  epi_stats="DD_DOWN_EPI" if sc and flags == "stats" else None,
                  slot=(lambda inp, i: _sliced(inp, i, ("x",)))
                  if flags != "stats" and B == DOWN_B else None,
                  scaled=("x",) if flags == "plain" and bf16 and B == DOWN_B else None)


def _dn_unit(ho, wo, cout, unit, ops, B=DOWN_B):
    cin = DOWN_CIN
    gs, nst = _down_gs(ho, wo, B), B - 1
    G = -(-B // gs)
    bf16 = ops == "bf16x3"

    def build(g):
        r = lambda *s: torch.randn(*s, generator=g)  # noqa: E731
        return {"yp": r(B, cin, 2 * ho, 2 * wo), "res": r(B, cin, 2 * ho, 2 * wo),
                "sc": torch.rand(G, cin, generator=g) + 0.5, "sh": r(G, cin) * 0.3,
                "w3": r(cout, cin, 3, 3) / (3 * cin ** 0.5), "w1": r(cout, cin, 1, 1) / cin ** 0.5,
                "gamma": torch.rand(cout, generator=g) + 0.5, "beta": r(cout)}

    def run(inp, dev):
        t = lambda k: inp[k].to(dev)  # noqa: E731
        with poisoned():
            p3 = _capi.conv3x3_pack(t("w3"), operands=ops)
            p1 = _capi.conv1x1_pack(t("w1"), operands=ops) if unit else None
            y, ys, st, sts = _capi.conv_down_unit_input(
                t("yp"), (t("sc"), t("sh")), p3, cout, gs, packed1x1=p1,
                residual=t("res") if unit else None, n_stat=nst)
        out = {"y": y, "stats": st.buf, "_st": st}
        if unit:
            out.update(y_sc=ys, stats_sc=sts.buf, _sts=sts)
        return out

    def ref(inp, out):
        x = inp["yp"].double() * ex(inp["sc"], gs, B) + ex(inp["sh"], gs, B)
        if unit:
            x = x + inp["res"].double()
        x = torch.relu(x)
        ident = lambda z: z  # noqa: E731
        res = {"y": _both(lambda a, b: F.conv2d(a, b, stride=2, padding=1), x, inp["w3"], ident,
                          bf16)}
        if unit:
            res["y_sc"] = _both(lambda a, b: F.conv2d(a, b, stride=2), x, inp["w1"], ident, bf16)
        return res

    tag = "" if B == DOWN_B else f"-b{B}"
    return Launch(f"dnu-{ho}x{wo}-c{cout}-{'unit' if unit else 'bn'}-{ops}{tag}", "down", ops, build,
                  run, ref,
                  stats=[("_st", "y", gs, nst)] + ([("_sts", "y_sc", gs, nst)] if unit else []))


DOWN_BWD_COUT, DOWN_BWD_CIN = 40, 70  # dh channels (K), dx channels (two ragged 64-blocks)


def _dn_bwd(ho, wo, dz, mask):
    B, cout, cin = DOWN_B, DOWN_BWD_COUT, DOWN_BWD_CIN
    shape = (B, cin, 2 * ho, 2 * wo)

    def build(g):
        r = lambda *s: torch.randn(*s, generator=g)  # noqa: E731
        return {"dh": r(B, cout, ho, wo), "dz": r(B, cout, ho, wo),
                "w3": r(cout, cin, 3, 3) / (3 * cout ** 0.5), "w1": r(cout, cin, 1, 1) / cout ** 0.5,
                "msk": r(*shape)}

    def run(inp, dev):
        t = lambda k: inp[k].to(dev)  # noqa: E731
        kw = {}
        if mask == "src":
            kw["mask_src"] = t("msk")
        elif mask == "bits":
            kw["mask_bits"] = plane_bits(inp["msk"] > 0).to(dev)
        with poisoned():
            p3 = _capi.conv3x3_pack(t("w3"), transpose_flip=True)
            p1 = _capi.conv1x1_pack(t("w1"), transpose=True) if dz else None
            dx = _capi.down_backward(t("dh"), p3, cin, dz=t("dz") if dz else None,
                                     packed1x1_t=p1, **kw)
        return {"dx": dx}

    def ref(inp, out):
        n1 = inp["dh"].shape[0]
        shp = (n1,) + shape[1:]

        def lin(a, b):  # a = [dh | dz] along channels, b = [w3 | w1 padded to 3x3]
            v = torch.nn.grad.conv2d_input(shp, b[:cout], a[:, :cout], stride=2, padding=1)
            if dz:
                v = v + torch.nn.grad.conv2d_input(shp, b[cout:, :, 1:2, 1:2], a[:, cout:],
                                                   stride=2)
            return v
        a = torch.cat([inp["dh"], inp["dz"]], 1).double()
        b = torch.cat([inp["w3"], F.pad(inp["w1"], (1, 1, 1, 1))], 0)
        keep = (inp["msk"] > 0) if mask != "none" else 1.0
        return {"dx": _both(lin, a, b, lambda z: z * keep, True)}

    return Launch(f"dnb-{ho}x{wo}-{'dz' if dz else 'nodz'}-{mask}", "down", "bf16x3", build, run,
                  ref, slot=lambda inp, i: _sliced(inp, i, ("dh", "dz", "msk")),
                  scaled=("dh", "dz") if mask == "none" else None,
                  # dd_down_backward refuses plane bits on the 64-position kernel
                  skip_env={"DD_DOWN_BWD": "1"} if mask == "bits" else None)


def _down_launches():
    out = []
    for ho, wo in DOWN_OUT:
        for cout in (40, 70):
            for sc in (True, False):
                for flags in DOWN_FLAGS:
                    for ops in ("bf16x3", "f16x3"):
                        if flags == "plain" and ops == "f16x3":
                            continue
                        out.append(_dn(ho, wo, cout, sc, flags, ops))
            for unit in (True, False):
                for ops in ("bf16x3", "f16x3"):
                    out.append(_dn_unit(ho, wo, cout, unit, ops))
        # two groups: per-group affine rows and statistics slots
        B2 = 7 if (ho, wo) == (4, 4) else 5
        out.append(_dn(ho, wo, 70, True, "stats", "bf16x3", B=B2))
        out.append(_dn_unit(ho, wo, 70, True, "bf16x3", B=B2))
        for dz in (True, False):
            for mask in ("none", "src", "bits"):
                if mask == "bits" and not _capi.down_backward_mask_bits_supported(ho, wo):
                    continue
                out.append(_dn_bwd(ho, wo, dz, mask))
    # more tiles than the forward's persistent grid (two workgroups per CU of a 256-CU device;
    # one tile per example and row block here): the tile walk and its XCD order
    out.append(_dn(8, 8, 70, True, "stats", "bf16x3", B=DOWN_MANY))
    out.append(_dn(2, 32, 40, True, "grand", "bf16x3", B=DOWN_MANY))
    return out


# ---- 1x1 / implicit GEMM ---------------------------------------------------------------------
# (B, cin, cout, H, W, stride); the 3x3 map runs the scalar mode (h w % 4 != 0)
C1_SHAPES = [(3, 20, 40, 8, 8, 1), (3, 20, 70, 8, 8, 1), (3, 20, 200, 8, 8, 1),
             (3, 20, 200, 8, 8, 2), (2, 20, 70, 3, 3, 1)]
# every code of DD_C1_SPEC_LIST, (epilogue, operand types), and bias + residual + ReLU
C1_EPI = [("stats", ("bf16x3", "f16x3")), ("stats_aff", ("bf16x3", "f16x3")),
          ("bias", ("f16x3",)), ("bias_relu", ("f16x3",)), ("msk", ("bf16x3",)),
          ("res_msk", ("bf16x3",)), ("up2_msk", ("bf16x3",)), ("plain", ("bf16x3", "f16x3")),
          ("brr", ("bf16x3", "f16x3"))]
# more tiles than resident workgroups (two per CU; one per CU on the 256-output family)
C1_COUNTS = [((1100, 20, 70, 8, 8, 1), "plain"), ((1100, 20, 70, 8, 8, 1), "stats"),
             ((600, 20, 200, 8, 8, 1), "plain"), ((13, 20, 40, 16, 8, 1), "plain")]


def gemm_gs(B, hw):
    """The smallest group size past B whose positions fill whole 128-position tiles."""
    step = 128 // math.gcd(128, hw)
    return step * (B // step + 1)


def _gemm(tag, shape, k, stride, pad, epi, ops, big=False, gs=None):
    """conv1x1 (k = 1) or conv_gemm (k x k) with one epilogue set."""
    B, cin, cout, H, W = shape
    ho, wo = (H + 2 * pad - k) // stride + 1, (W + 2 * pad - k) // stride + 1
    grouped = epi in ("stats", "stats_aff")
    gs = (gs or (gemm_gs(B, ho * wo) if not big else 64)) if grouped else None
    G = -(-B // gs) if grouped else 1
    nst = B - 1
    bf16 = ops == "bf16x3"
    oshape = (B, cout, ho, wo)

    def build(g):
        r = lambda *s: torch.randn(*s, generator=g)  # noqa: E731
        d = {"x": r(B, cin, H, W), "w": r(cout, cin, k, k) / (k * cin ** 0.5)}
        if not big:
            d.update(bias=r(cout), res=r(*oshape), msk=r(*oshape),
                     up2=r(B, cout, ho // 2, wo // 2), sc=torch.rand(G, cin, generator=g) + 0.5,
                     sh=r(G, cin) * 0.3)
        d.update(gamma=torch.rand(cout, generator=g) + 0.5, beta=r(cout))
        return d

    def run(inp, dev):
        t = lambda n: inp[n].to(dev)  # noqa: E731
        kw = {}
        if epi in ("bias", "bias_relu", "brr"):
            kw["bias"] = t("bias")
        if epi in ("bias_relu", "brr"):
            kw["relu"] = True
        if epi in ("res_msk", "brr"):
            kw["residual"] = t("res")
        if epi in ("msk", "res_msk", "up2_msk"):
            kw["mask_src"] = t("msk")
        if epi == "up2_msk":
            kw["res_up2"] = t("up2")
        if grouped:
            kw.update(stats=True, group_size=gs, n_stat=nst)
        if epi == "stats_aff":
            kw["in_affine"] = (t("sc"), t("sh"))
        with poisoned():
            if k == 1:
                pk = _capi.conv1x1_pack(t("w"), operands=ops)
                y = _capi.conv1x1(t("x"), pk, cout, stride=stride, **kw)
            else:
                pk = _capi.conv_gemm_pack(t("w"), operands=ops)
                y = _capi.conv_gemm(t("x"), pk, cout, k, stride, pad, **kw)
        if grouped:
            return {"y": y[0], "stats": y[1].buf, "_st": y[1]}
        return {"y": y}

    def ref(inp, out):
        x = inp["x"].double()
        if epi == "stats_aff":
            x = torch.relu(x * ex(inp["sc"], gs, B) + ex(inp["sh"], gs, B))

        def e(z):
            if "bias" in epi or epi == "brr":
                z = z + inp["bias"].double()[None, :, None, None]
            if epi in ("res_msk", "brr"):
                z = z + inp["res"].double()
            if epi == "up2_msk":
                up = torch.zeros(oshape, dtype=torch.float64)
                up[:, :, ::2, ::2] = inp["up2"].double()
                z = z + up
            if epi in ("bias_relu", "brr"):
                z = torch.relu(z)
            if epi.endswith("msk"):
                z = z * (inp["msk"] > 0)
            return z
        return {"y": _both(lambda a, b: F.conv2d(a, b, stride=stride, padding=pad), x, inp["w"],
                           e, bf16)}

    return Launch(f"{tag}-{'x'.join(map(str, shape))}-k{k}s{stride}-{epi}-{ops}", "c1x1", ops,
                  build, run, ref, stats=[("_st", "y", gs, nst)] if grouped else (), big=big,
                  # launch_cfg: the float4 1x1 mode is the one with specialised epilogues
                  epi_stats="DD_C1_EPI" if grouped and k == 1 and (ho * wo) % 4 == 0 else None)


def _c1_unit(shape, mode, ops, gs=None):
    B, cin, cout, H, W = shape
    gs, nst = gs or gemm_gs(B, H * W), B - 1
    G = -(-B // gs)
    bf16 = ops == "bf16x3"

    def build(g):
        r = lambda *s: torch.randn(*s, generator=g)  # noqa: E731
        return {"yp": r(B, cin, H, W), "res": r(B, cin, H, W),
                "sc": torch.rand(G, cin, generator=g) + 0.5, "sh": r(G, cin) * 0.3,
                "rsc": torch.rand(G, cin, generator=g) + 0.5, "rsh": r(G, cin) * 0.3,
                "w": r(cout, cin, 1, 1) / cin ** 0.5,
                "gamma": torch.rand(cout, generator=g) + 0.5, "beta": r(cout)}

    def run(inp, dev):
        t = lambda n: inp[n].to(dev)  # noqa: E731
        with poisoned():
            pk = _capi.conv1x1_pack(t("w"), operands=ops)
            xo, y, st = _capi.conv1x1_unit_input(
                t("yp"), (t("sc"), t("sh")), pk, cout, gs, n_stat=nst,
                residual=t("res") if mode != "none" else None,
                res_affine=(t("rsc"), t("rsh")) if mode == "affine" else None)
        return {"x_out": xo, "y": y, "stats": st.buf, "_st": st}

    def ref(inp, out):
        x = inp["yp"].double() * ex(inp["sc"], gs, B) + ex(inp["sh"], gs, B)
        if mode == "raw":
            x = x + inp["res"].double()
        elif mode == "affine":
            x = x + inp["res"].double() * ex(inp["rsc"], gs, B) + ex(inp["rsh"], gs, B)
        x = torch.relu(x)
        return {"x_out": (x, None),
                "y": _both(lambda a, b: F.conv2d(a, b), x, inp["w"], lambda z: z, bf16)}

    return Launch(f"c1u-{'x'.join(map(str, shape))}-{mode}-{ops}", "c1x1", ops, build, run, ref,
                  stats=[("_st", "y", gs, nst)])


def _c1x1_launches():
    out = []
    for (B, cin, cout, H, W, s) in C1_SHAPES:
        for epi, opss in C1_EPI:
            if epi == "up2_msk" and ((H // s) % 2 or (W // s) % 2):
                continue
            for ops in opss:
                out.append(_gemm("c1", (B, cin, cout, H, W), 1, s, 0, epi, ops))
        if s == 1 and (H * W) % 4 == 0:
            for mode in ("none", "raw", "affine"):
                for ops in ("bf16x3", "f16x3"):
                    out.append(_c1_unit((B, cin, cout, H, W), mode, ops))
    for ops in ("bf16x3", "f16x3"):
        # 20 channels take the dense-K pack (no staging transform there), 40 the tap-major mode
        for epi in ("plain", "brr", "stats"):
            out.append(_gemm("gemm3", (2, 20, 70, 9, 11), 3, 1, 1, epi, ops))
        for epi in ("plain", "brr", "stats", "stats_aff"):
            out.append(_gemm("gemm3", (2, 40, 70, 9, 11), 3, 1, 1, epi, ops))
        for epi in ("plain", "bias_relu", "stats"):
            out.append(_gemm("stem7", (2, 3, 64, 30, 40), 7, 2, 3, epi, ops))
    # two groups: per-group affine rows and statistics slots
    for ops in ("bf16x3", "f16x3"):
        out.append(_gemm("c1", (6, 20, 70, 8, 8), 1, 1, 0, "stats_aff", ops, gs=4))
        out.append(_gemm("c1", (11, 20, 200, 8, 8), 1, 2, 0, "stats_aff", ops, gs=8))
    out.append(_c1_unit((6, 20, 70, 8, 8), "affine", "bf16x3", gs=4))
    for (B, cin, cout, H, W, s), epi in C1_COUNTS:
        out.append(_gemm("c1", (B, cin, cout, H, W), 1, s, 0, epi, "bf16x3", big=True))
    return out


def _build_list():
    out = _conv3x3_launches() + _down_launches() + _c1x1_launches()
    names = [la.name for la in out]
    assert len(set(names)) == len(names), "launch names must be unique"
    return out


LAUNCHES = _build_list()


def launches(family):
    return [la for la in LAUNCHES if la.family == family]
