"""One list of named launches of the GraNd per-example norm kernels (dd_conv_pegrad_sqnorm: every
kernel instance its dispatch can reach, each at the smallest ragged shape that reaches it;
dd_linear_pegrad_sqnorm; dd_bn_pegrad_sqnorm), the probes each launch carries and their float64
references, for tests/test_pegrad_probes.py (CPU: the probes separate a damaged kernel from a
sound one) and tests/test_gpu_pegrad_probes.py (the kernels themselves).  Data and small
functions only.

A norm is one scalar per example, and a sum of squares over 9 cin cout weight-gradient entries
averages element errors away: on dense iid data a kernel that lost a lo product of the bf16
split, or one channel of a ragged tail, stays inside rtol 1e-3.  So example b of a batch is one
probe:
  pair      act non-zero in one input channel, gout in one output channel (normal + 3, normal);
            the pairs cross both sides' tile edges (0, 15, 16, 31, 32, 63, 64, last)
  2x2       two channels on each side, straddling a block edge: sums happen before the square
  pos       one channel pair, act restricted to one row or column (first, last, both sides of a
            step boundary) or, at stride 2, to one parity class of rows or columns
  dense     relu(normal) x 1e-2 normal over all channels, as the older tests
  zero_*    an all-zero act or gout: the example adds exactly 0.0
Every probe has
  ref       the exact norm (oracle.pegrad, float64)
  e3        the norm in the arithmetic the kernel's source states, summed in float64: bf16 hi/lo
            halves and the products hi.hi + hi.lo + lo.hi (direct forms: on U and G; Gram forms:
            on each Gram P = a^T a, K_g = g^T g, then the tap gather), col_scale applied where
            the kernel applies it; for the fp32 kernels a CPU float32 restatement
  damaged   e3 with a lo product dropped (no_lh: a_lo.g_hi, no_hl: a_hi.g_lo, hh: both, plain
            bf16); for the fp32 kernels the operands rounded to bf16
The error of an output is the max over examples of |sq / ref - 1|.  A kernel is held to
K x err(e3) + FLOOR (bound()) on each group of probes by itself: the pairs, the position probes,
and the rest (2x2 and dense).
"""
import functools
import types

import numpy as np
import torch
import torch.nn.functional as F

from data_diet_distributed_amd import _capi
from helpers.conv_launches import _split, seed_of
from oracle import pegrad as o_pegrad

FAMILIES = ("fp32", "direct3x3", "direct1x1", "gram", "stem", "linear", "bn")
# every kernel instance the dispatch can reach (pgram_kernel<32, 64> cannot be reached: no
# geometry the dispatcher admits has more output than input positions).  conv_method names the
# family only: that a launch reaches the instance in its name (the p or w kernel, the LC layout,
# the pgram<Ti, To> and BN variants) is checked by the recorded kernel trace alone
# (profiles/pegrad_probes/README.md); when d1x1_layout or direct3x3_wide change, record it anew
INSTANCES = (
    "pegrad_direct_kernel", "pegrad_ghost16_kernel", "pegrad_ghost64_kernel",
    "pegrad_direct3x3_kernel<32,1>", "pegrad_direct3x3_kernel<8,1>",
    "pegrad_direct3x3p_kernel<16,1>", "pegrad_direct3x3p_kernel<16,2>",
    "pegrad_direct3x3w_kernel<16,1>", "pegrad_direct3x3w_kernel<16,2>",
    "pegrad_direct1x1_kernel<1,1>", "pegrad_direct1x1_kernel<1,2>",
    "pegrad_direct1x1_kernel<1,4>", "pegrad_direct1x1_kernel<2,1>",
    "pegrad_direct1x1_kernel<2,2>", "pegrad_direct1x1_kernel<2,4>",
    "pgram_kernel<64,64>", "pgram_kernel<64,32>", "pgram_kernel<32,32>", "pgram_par_kernel",
    "pgram_q_kernel", "stem_kernel<8>", "stem_kernel<16>", "stem_kernel<32>",
    "linear_pegrad_kernel", "bn_pegrad_kernel<4,true>", "bn_pegrad_kernel<16,true>",
    "bn_pegrad_kernel<64,true>", "bn_pegrad_kernel<64,false>",
)
PERSISTENT = tuple(i for i in INSTANCES if "3x3p" in i or "3x3w" in i)
CUS = 256  # workgroups of a persistent grid on the MI355X: a hand-over launch has more tiles

# 16 fp32 ulps: the final fp32 adds of the partials
FLOOR = 2.0 ** -20
# 1.5 x the largest kernel / e3 ratio measured on the MI355X over every group of probes of every
# launch, per arithmetic, rounded up to two decimals (profiles/pegrad_probes/README.md: bf16x3
# 0.703 to 1.192 over 120 groups; fp32 0.113 to 3.485 over 46, two fp32 roundings of a few ulps
# each, below FLOOR on all but the 1x1 launches)
K = {"bf16x3": 1.79, "fp32": 5.23}

EDGES = (0, 15, 16, 31, 32, 63, 64)
BF16_VARIANTS = ("no_lh", "no_hl", "hh")
F32_VARIANTS = ("bf16",)


def edges(n):
    return sorted({e for e in EDGES if e < n} | {n - 1})


def straddle(n):
    for e in (64, 32, 16):
        if n > e:
            return [e - 1, e]
    return sorted({0, n - 1})


def err(sq, ref):
    """max over the examples with a non-zero norm of |sq / ref - 1|"""
    sq, ref = np.asarray(sq, np.float64), np.asarray(ref, np.float64)
    nz = ref != 0
    return float(np.abs(sq[nz] / ref[nz] - 1).max())


def bound(la, case, mask=None):
    """of the examples in mask (all: the launch's bound); the tests hold each group of probes
    (case.groups) to its own, so the ill-conditioned position probes of a 1x1 launch do not set
    the bar of its pairs"""
    mask = slice(None) if mask is None else mask
    return K[la.arith] * err(case.e3[mask], case.ref[mask]) + FLOOR


def xcd_remap(orig, nwg):
    """the logical tile of workgroup-order tile orig (dd_pegrad.hip)"""
    q, r, xcd = nwg // 8, nwg % 8, orig % 8
    return (xcd * (q + 1) if xcd < r else r * (q + 1) + (xcd - r) * q) + orig // 8


class Launch:
    """name, family, instance (the kernel the name says it reaches), arith ("bf16x3" | "fp32"),
    batched (input keys with a batch dimension), homog ({input key: (log2 of its scale, log2 of
    the norm's)}), env ({knob: value} read per call), handover (more tiles than workgroups)."""
    env = {}
    handover = False

    def __repr__(self):
        return self.name

    def case(self):
        return _case(self)


# ---- float64 / float32 restatements of one example --------------------------------------------
def _cols(a, la):
    """[C, H, W] -> im2col [C k k, T]"""
    return F.unfold(a[None], (la.k, la.k), padding=la.pad, stride=la.stride)[0]


def _three(u_h, u_l, v_h, v_l, var, mul):
    r = mul(u_h, v_h)
    if var in ("e3", "no_lh"):
        r = r + mul(u_h, v_l)
    if var in ("e3", "no_hl"):
        r = r + mul(u_l, v_h)
    return r


def _emu_direct(la, a, g, s, var):
    """U_hi G_hi + U_hi G_lo + U_lo G_hi; the squared column sums times fp32(s_o * s_o) (the
    stem splits fp32(g * s_o) instead)."""
    g = g.reshape(len(g), -1)
    if la.form == "stem" and s is not None:
        g, s = g * s[:, None], None
    ah, al = _split(a)
    gh, gl = _split(g)
    W = _three(_cols(ah, la), _cols(al, la), gh, gl, var, lambda u, v: u @ v.T)
    q = (W * W).sum(0)
    if s is not None:
        q = q * (s * s).double()
    return q.sum().item()


@functools.lru_cache(maxsize=None)
def _tap_index(h, w, k, stride, pad):
    """[k k, To] input position each tap of each output reads; h w (a zero row) for padding"""
    pos = torch.arange(h * w, dtype=torch.float64).reshape(1, h, w) + 1
    idx = F.unfold(pos[None], (k, k), padding=pad, stride=stride)[0].long() - 1
    idx[idx < 0] = h * w
    return idx


def _emu_gram(la, a, g, s, var):
    """K_g = g^T g over fp32(g * s_o), P = a^T a, each in the three products of its operands'
    halves; K_a gathers P per tap; sum K_a K_g."""
    g = g.reshape(len(g), -1)
    if s is not None:
        g = g * s[:, None]
    gram = lambda x: _three(*(2 * _split(x)), var, lambda u, v: u.T @ v)
    Kg = gram(g)
    Pp = F.pad(gram(a.reshape(len(a), -1)), (0, 1, 0, 1))
    Ka = sum(Pp[i[:, None], i[None, :]] for i in _tap_index(la.h, la.w, la.k, la.stride, la.pad))
    return (Ka * Kg).sum().item()


def _emu_f32(la, a, g, s, var):
    """the kernel's contraction in CPU float32 (var "bf16": on operands rounded to bf16)"""
    g = g.reshape(len(g), -1)
    if var == "bf16":
        a, g = a.bfloat16().float(), g.bfloat16().float()
    U = _cols(a, la)
    if la.form == "f32direct":
        W = U @ g.T
        q = (W * W).sum(0)
        if s is not None:
            q = q * (s * s)
        return q.sum().item()
    if s is not None:
        g = g * s[:, None]
    return ((U.T @ U) * (g.T @ g)).sum().item()


_EMU = {"direct": _emu_direct, "stem": _emu_direct, "gram": _emu_gram, "f32direct": _emu_f32,
        "f32ghost": _emu_f32}


# ---- conv launches ----------------------------------------------------------------------------
class Conv(Launch):
    batched = ("act", "gout")
    # magnitudes: |act| < 8, |gout| in (1e-9, 6): halves, products and squares of 2^5 act and
    # 2^-12 gout stay far inside the normal range of bf16 and fp32
    homog = {"gout": (-12, -24), "act": (5, 10)}

    def __init__(self, name, family, instance, kernel, form, cin, h, w, cout, k=3, stride=1,
                 pad=1, method="direct", prec="bf16x3", scale=False, wide=None, B=None):
        self.name, self.family, self.instance, self.kernel = name, family, instance, kernel
        self.form, self.cin, self.h, self.w, self.cout = form, cin, h, w, cout
        self.k, self.stride, self.pad, self.method, self.prec = k, stride, pad, method, prec
        self.scale, self.B = scale, B
        self.arith = prec
        self.variants = BF16_VARIANTS if prec == "bf16x3" else F32_VARIANTS
        self.ho, self.wo = (h + 2 * pad - k) // stride + 1, (w + 2 * pad - k) // stride + 1
        self.env = {} if wide is None else {"DD_PEGRAD_WIDE": str(wide)}
        self.handover = B is not None

    def geom(self, B):
        return _capi.ConvGeom(B, self.cin, self.h, self.w, self.cout, self.ho, self.wo, self.k,
                              self.k, self.stride, self.pad)

    def tiles(self, B):
        """workgroup tiles of a persistent launch"""
        return B * self._per_example()[0]

    def _per_example(self):
        nob = -(-self.cout // 64)
        nblk = (nob + 1) // 2 if "3x3w" in self.instance else nob  # o-blocks of workgroup tiles
        return -(-self.cin // 64) * nblk, nblk

    def handovers(self, B):
        """((c-block, o-block) of a tile, of its workgroup's next tile) for every hand-over of
        the persistent launch at batch B (set_tile of dd_pegrad.hip)"""
        per_ex, nblk = self._per_example()
        total = B * per_ex
        where = lambda t: divmod(xcd_remap(t, total) % per_ex, nblk)
        return [(where(t), where(t + CUS)) for t in range(max(0, total - CUS))]

    def workspace_bytes(self, B):
        return _capi.conv_workspace_bytes(self.geom(B), self.method, self.prec)

    def launch(self, t, sq, ws):
        _capi.conv_pegrad_sqnorm(t["act"], t["gout"], (self.k, self.k), self.stride, self.pad, sq,
                                 ws, method=self.method, precision=self.prec,
                                 col_scale=t.get("col_scale"))

    def _pos_masks(self):
        """[h, w] masks of the position probes"""
        h, w, out = self.h, self.w, []
        # input rows a step of the direct 3x3 kernels consumes (else half the map)
        sr = self.stride * max(1, 32 // self.wo) if self.family == "direct3x3" else max(1, h // 2)
        for r in sorted({0, h - 1} | {r for r in (sr - 1, sr) if r < h}):
            m = torch.zeros(h, w)
            m[r] = 1
            out.append(m)
        for c in sorted({0, w - 1}):
            m = torch.zeros(h, w)
            m[:, c] = 1
            out.append(m)
        if self.stride == 2:
            for par in (0, 1):
                m = torch.zeros(h, w)
                m[par::2] = 1
                out.append(m)
                m = torch.zeros(h, w)
                m[:, par::2] = 1
                out.append(m)
        return out

    def build(self, rng):
        cin, cout = self.cin, self.cout
        allc, allo = list(range(cin)), list(range(cout))
        pairs = [("pair", [c], [o], None) for c in edges(cin) for o in edges(cout)]
        specs = list(pairs)
        specs.append(("2x2", straddle(cin), straddle(cout), None))
        specs += [("pos", [cin - 1], [cout - 1], m) for m in self._pos_masks()]
        specs.append(("dense", allc, allo, None))
        specs += [("zero_act", [0], allo, None), ("zero_gout", allc, [0], None)]
        i = 0
        while len(specs) < (self.B or 0) or len(specs) % 8 == 0:  # (pgram_q: B % 8 != 0)
            specs.append(pairs[(7 * i + 3) % len(pairs)])
            i += 1
        B = len(specs)
        act = torch.zeros(B, cin, self.h, self.w)
        gout = torch.zeros(B, cout, self.ho, self.wo)
        normal = lambda *shape: torch.from_numpy(rng.normal(size=shape).astype(np.float32))
        for b, (kind, cs, os_, mask) in enumerate(specs):
            if kind == "dense":
                act[b] = normal(cin, self.h, self.w).clamp_min(0)
                gout[b] = 1e-2 * normal(cout, self.ho, self.wo)
                continue
            if kind != "zero_act":
                a = normal(len(cs), self.h, self.w) + 3
                act[b, cs] = a if mask is None else a * mask
            if kind != "zero_gout":
                gout[b, os_] = normal(len(os_), self.ho, self.wo)
        inp = {"act": act, "gout": gout}
        if self.scale:
            # neighbouring 64-output blocks differ by factors of 4 (0.25, 1, 4) times a random
            # factor: a tile that took another block's scales or output index is far off
            blk = torch.tensor([0.25, 1.0, 4.0])[(torch.arange(cout) // 64) % 3]
            inp["col_scale"] = blk * torch.from_numpy(
                rng.uniform(0.5, 1.5, size=cout).astype(np.float32))
        return inp, [(k_, cs, os_) for k_, cs, os_, _ in specs]

    def refs(self, inp, specs):
        s_all = inp.get("col_scale")
        emu = _EMU[self.form]
        cols = {v: [] for v in ("ref", "e3") + self.variants}
        for b, (kind, cs, os_) in enumerate(specs):
            a, g = inp["act"][b, cs], inp["gout"][b, os_]
            s = None if s_all is None else s_all[os_]
            cols["ref"].append(o_pegrad.conv_pegrad_sqnorm(
                a[None].numpy(), g[None].numpy(), self.k, self.k, self.stride, self.pad,
                col_scale=None if s is None else s.numpy())[0])
            for v in ("e3",) + self.variants:
                cols[v].append(emu(self, a, g, s, v))
        return cols


# ---- linear and batch-norm launches -----------------------------------------------------------
def _sq(x, dims):
    return (x * x).sum(dims)


class Linear(Launch):
    family, instance, arith, variants = "linear", "linear_pegrad_kernel", "fp32", F32_VARIANTS
    batched = ("act", "gout")
    homog = {"gout": (-12, -24)}

    def __init__(self, name, din, dout, bias):
        self.name, self.din, self.dout, self.bias = name, din, dout, bias

    def workspace_bytes(self, B):
        return 0

    def launch(self, t, sq, ws):
        _capi.linear_pegrad_sqnorm(t["act"], t["gout"], sq, self.bias)

    def build(self, rng):
        normal = lambda *shape: torch.from_numpy(rng.normal(size=shape).astype(np.float32))
        specs = [("pair", [c], [o]) for c in edges(self.din) for o in edges(self.dout)]
        specs += [("2x2", straddle(self.din), straddle(self.dout)), ("dense", None, None),
                  ("zero_gout", None, [])]
        if not self.bias:
            specs.append(("zero_act", [], None))
        act, gout = torch.zeros(len(specs), self.din), torch.zeros(len(specs), self.dout)
        for b, (kind, cs, os_) in enumerate(specs):
            cs = list(range(self.din)) if cs is None else cs
            os_ = list(range(self.dout)) if os_ is None else os_
            dense = kind == "dense"
            act[b, cs] = normal(len(cs)).clamp_min(0) if dense else normal(len(cs)) + 3
            gout[b, os_] = normal(len(os_)) * (1e-2 if dense else 1.0)
        return {"act": act, "gout": gout}, specs

    def refs(self, inp, specs):
        a, g = inp["act"], inp["gout"]
        out = {"ref": o_pegrad.linear_pegrad_sqnorm(a.numpy(), g.numpy(), self.bias)}
        for v, f in (("e3", lambda x: x), ("bf16", lambda x: x.bfloat16().float())):
            a2, g2 = _sq(f(a), 1), _sq(f(g), 1)
            out[v] = (a2 * g2 + (g2 if self.bias else 0.0)).double().numpy()
        return out


class BN(Launch):
    family, arith, variants = "bn", "fp32", F32_VARIANTS
    homog = {"g": (-12, -24)}

    def __init__(self, name, C, h, w, res):
        self.name, self.C, self.h, self.w, self.res = name, C, h, w, res
        hw = h * w
        self.instance = "bn_pegrad_kernel<%s>" % (
            "64,false" if hw % 4 else "4,true" if hw <= 16 else "16,true" if hw <= 64
            else "64,true")
        self.batched = ("v", "g", "r") if res else ("v", "g")

    def workspace_bytes(self, B):
        return 0

    def launch(self, t, sq, ws):
        _capi.bn_pegrad_sqnorm(t["v"], t["g"], t["gamma"], t["beta"], sq, r=t.get("r"))

    def build(self, rng):
        C, h, w = self.C, self.h, self.w
        normal = lambda *shape: torch.from_numpy(rng.normal(size=shape).astype(np.float32))
        specs = [("pair", [c]) for c in edges(C)] + [("2x2", straddle(C))]
        specs += [("pos", [C - 1]), ("dense", list(range(C))), ("zero_g", [])]
        B = len(specs)
        gamma = torch.from_numpy(rng.uniform(0.5, 1.5, size=C).astype(np.float32))
        gamma[1::2] *= -1
        beta = 0.1 * normal(C)
        inp = {"v": normal(B, C, h, w) * gamma[:, None, None] + beta[:, None, None],
               "g": torch.zeros(B, C, h, w), "gamma": gamma, "beta": beta}
        if self.res:
            inp["r"] = normal(B, C, h, w)
            inp["v"] = inp["v"] + inp["r"]
        for b, (kind, cs) in enumerate(specs):
            inp["g"][b, cs] = normal(len(cs), h, w) * (1e-2 if kind == "dense" else 1.0)
            if kind == "pos":
                keep = torch.zeros(h, w)
                keep[h - 1, w - 1] = 1
                inp["g"][b] *= keep
        return inp, specs

    def refs(self, inp, specs):
        v, g, ga, be = inp["v"], inp["g"], inp["gamma"], inp["beta"]
        r = inp.get("r")
        out = {"ref": o_pegrad.bn_pegrad_sqnorm(
            v.double().numpy() - (0 if r is None else r.double().numpy()), g.numpy(),
            ga.numpy(), be.numpy())}
        for name, f in (("e3", lambda x: x), ("bf16", lambda x: x.bfloat16().float())):
            x = f(v) - (0 if r is None else f(r)) - be[:, None, None]
            dg = (f(g) * x).sum((2, 3)) / ga
            out[name] = (_sq(dg, 1) + _sq(f(g).sum((2, 3)), 1)).double().numpy()
        return out


@functools.lru_cache(maxsize=None)
def _case(la):
    """The launch's inputs (CPU tensors), probe kinds and references; computed once, shared."""
    inp, specs = la.build(np.random.default_rng(seed_of(la.name)))
    c = types.SimpleNamespace(inp=inp, kinds=[s[0] for s in specs], B=len(specs))
    for k_, v in la.refs(inp, specs).items():
        v = np.asarray(v, np.float64)
        v.setflags(write=False)
        setattr(c, k_, v)
    c.damaged = {v: getattr(c, v) for v in la.variants}
    c.pair = np.array([k_ == "pair" for k_ in c.kinds])
    # the zero probes, and the position probes a stride-2 1x1 never reads (its odd rows and
    # columns): an exact 0.0
    c.zero = c.ref == 0
    assert all(z for z, k_ in zip(c.zero, c.kinds) if k_.startswith("zero"))
    assert not any(z for z, k_ in zip(c.zero, c.kinds) if k_ in ("pair", "2x2", "dense"))
    pos = np.array([k_ == "pos" for k_ in c.kinds])
    # the groups of probes that carry a bound of their own
    c.groups = {n: m & ~c.zero for n, m in (("pair", c.pair), ("pos", pos),
                                            ("rest", ~c.pair & ~pos)) if (m & ~c.zero).any()}
    return c


# ---- the list ---------------------------------------------------------------------------------
def _conv_launches():
    out = []

    def add(name, *a, **k):
        out.append(Conv(name, *a, **k))

    f32 = dict(prec="fp32")
    add("fp32-direct-3x3-c17-o40-7x6", "fp32", "pegrad_direct_kernel", "direct", "f32direct",
        17, 7, 6, 40, scale=True, **f32)
    add("fp32-direct-1x1s2-c70-o130-7x7", "fp32", "pegrad_direct_kernel", "direct", "f32direct",
        70, 7, 7, 130, k=1, stride=2, pad=0, **f32)
    add("fp32-ghost16-3x3-c17-o40-4x4", "fp32", "pegrad_ghost16_kernel", "ghost", "f32ghost",
        17, 4, 4, 40, method="ghost", scale=True, **f32)
    add("fp32-ghost16-1x1-c70-o17-3x3", "fp32", "pegrad_ghost16_kernel", "ghost", "f32ghost",
        70, 3, 3, 17, k=1, pad=0, method="ghost", **f32)
    add("fp32-ghost64-3x3-c17-o40-9x9-nT2", "fp32", "pegrad_ghost64_kernel", "ghost", "f32ghost",
        17, 9, 9, 40, method="ghost", scale=True, **f32)
    add("fp32-ghost64-1x1-c70-o17-9x8-nT2", "fp32", "pegrad_ghost64_kernel", "ghost", "f32ghost",
        70, 9, 8, 17, k=1, pad=0, method="ghost", **f32)

    # direct 3x3: H == R (one step per tile), H == 2R, H == 3R (an odd step count); the
    # persistent kernels' one- and two-step launches have more tiles than workgroups
    d3 = ("direct3x3", "direct", )
    for W, R in ((32, 1), (8, 4)):
        inst = f"pegrad_direct3x3_kernel<{W},1>"
        add(f"d3x3<{W},1>-c70-o130-{R}x{W}-1step", "direct3x3", inst, *d3, 70, R, W, 130,
            scale=True)
        add(f"d3x3<{W},1>-c17-o40-{3 * R}x{W}-3steps", "direct3x3", inst, *d3, 17, 3 * R, W, 40)
    # A workgroup's next tile is 256 on: logical tile + 32.  Three c-blocks make that a change
    # of o-block under the 64-wide tile (9 tiles per example) but only of c-block under the wide
    # one (6: its two o-blocks per c-block never rotate at 130 outputs), so the wide kernel also
    # has launches at 300 outputs: 5 o-blocks, 3 wide tiles per c-block, the last half empty.
    # B = 201: the batch cut to its first third still has more tiles than workgroups
    for S in (1, 2):
        for kern, wide in (("p", 0), ("w", 1)):
            inst = f"pegrad_direct3x3{kern}_kernel<16,{S}>"
            tag = f"d3x3{kern}<16,{S}>"
            for steps in (1, 2):
                h = 2 * S * steps
                for cin, cout in ((130, 130),) + (((70, 300),) if wide else ()):
                    add(f"{tag}-c{cin}-o{cout}-{h}x{16 * S}-{steps}step-handover", "direct3x3",
                        inst, *d3, cin, h, 16 * S, cout, stride=S, scale=True, wide=wide, B=201)
            # (o130 under the wide tile: 3 o-blocks, the last wide tile half empty)
            add(f"{tag}-c17-o{200 if wide else 40}-{6 * S}x{16 * S}-3steps", "direct3x3", inst,
                *d3, 17, 6 * S, 16 * S, 200 if wide else 40, stride=S, wide=wide)

    # direct 1x1: channel counts that make d1x1_layout return each LC, two tiles along c
    for S, maps in ((1, ((6, 6), (7, 7), (6, 6))), (2, ((16, 8), (13, 13), (16, 8)))):
        for (LC, cin, cout), (h, w) in zip(((1, 120, 250), (2, 250, 120), (4, 500, 60)), maps):
            add(f"d1x1<{S},{LC}>-c{cin}-o{cout}-{h}x{w}" + ("-scalar" if h % 2 else ""),
                "direct1x1", f"pegrad_direct1x1_kernel<{S},{LC}>", "direct1x1", "direct", cin, h,
                w, cout, k=1, stride=S, pad=0, scale=LC == 2)

    g = dict(method="auto")
    add("pgram<64,64>-3x3-c70-o130-6x6", "gram", "pgram_kernel<64,64>", "pgram", "gram", 70, 6, 6,
        130, scale=True, **g)
    add("pgram<64,64>-1x1-c17-o40-6x6", "gram", "pgram_kernel<64,64>", "pgram", "gram", 17, 6, 6,
        40, k=1, pad=0, **g)
    add("pgram<64,64>-3x3-c260-o40-6x6-streamed", "gram", "pgram_kernel<64,64>", "pgram", "gram",
        260, 6, 6, 40, **g)
    add("pgram<64,32>-3x3s2-c70-o130-8x8", "gram", "pgram_kernel<64,32>", "pgram", "gram", 70, 8,
        8, 130, stride=2, **g)
    add("pgram<64,32>-1x1s2-c17-o40-8x8", "gram", "pgram_kernel<64,32>", "pgram", "gram", 17, 8, 8,
        40, k=1, stride=2, pad=0, scale=True, **g)
    add("pgram<32,32>-3x3-c70-o130-4x4", "gram", "pgram_kernel<32,32>", "pgram", "gram", 70, 4, 4,
        130, scale=True, **g)
    add("pgram<32,32>-1x1-c17-o40-4x6", "gram", "pgram_kernel<32,32>", "pgram", "gram", 17, 4, 6,
        40, k=1, pad=0, **g)
    add("pgram_par-3x3s2-c70-o130-16x16", "gram", "pgram_par_kernel", "pgram", "gram", 70, 16, 16,
        130, stride=2, scale=True, **g)
    add("pgram_par-1x1s2-c17-o40-16x16", "gram", "pgram_par_kernel", "pgram", "gram", 17, 16, 16,
        40, k=1, stride=2, pad=0, **g)
    add("pgram_q-3x3-c70-o130-16x16", "gram", "pgram_q_kernel", "pgram_q", "gram", 70, 16, 16, 130,
        method="ghost")
    add("pgram_q-3x3-c17-o40-16x16", "gram", "pgram_q_kernel", "pgram_q", "gram", 17, 16, 16, 40,
        method="ghost", scale=True)

    add("stem<8>-c3-o40-8x8", "stem", "stem_kernel<8>", "stem", "stem", 3, 8, 8, 40, **g)
    add("stem<16>-c2-o17-12x16", "stem", "stem_kernel<16>", "stem", "stem", 2, 12, 16, 17,
        scale=True, **g)
    add("stem<32>-c3-o40-4x32", "stem", "stem_kernel<32>", "stem", "stem", 3, 4, 32, 40,
        scale=True, **g)
    return out


def _build_list():
    out = _conv_launches()
    out += [Linear("linear-d70-o10-bias", 70, 10, True), Linear("linear-d130-o17", 130, 17, False)]
    for C, h, w in ((17, 4, 4), (70, 8, 8), (40, 16, 8), (17, 7, 7)):
        for res in (False, True):
            out.append(BN(f"bn-c{C}-{h}x{w}" + ("-res" if res else ""), C, h, w, res))
    names = [la.name for la in out]
    assert len(set(names)) == len(names), "launch names must be unique"
    return out


LAUNCHES = _build_list()
