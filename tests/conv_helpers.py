"""References, counted bounds, guarded buffers and case tables for the conv family: the CONV instantiations of the GEMM kernel through
lseg_op_conv_ex (forward, every tile and epilogue, split-K slabs), conv_reduce_pad, the K-major weight gradients and the weight packers.
Rounding, intervals, guards and comparisons are those of tests/gemm_helpers.py (imported, not copied).

Reference.  fp64 torch on the operands after their rounding to the operand type, written from the PyTorch operation: F.conv2d(x_padded, w,
bias, stride, padding=0) over the PADDED input for 3x3 (over the interior for 1x1), ReLU and the skips in the stated order; autograd of that
expression for the weight gradient; flip / transpose / permute of the 4-d weight for the packers.  The input map's one-pixel border holds
random NON-ZERO values: padding=0 over the padded map is what the kernel computes, and a read of the wrong border cell shows.

Bound, counted.  Products of two 16-bit values are exact in fp32; only additions round.  Sc = sum|x||w| + |bias| (fp64) bounds the
accumulator: bc = (K_range + 1) 2^-23 Sc, K_range = 9 Cin or Cin (a split range's own length for a slab, the padded pixel count for a
weight gradient).  Each skip is one more fp32 addition: ba = nres 2^-23 (|t| + |res| + |res2|), t the value the skips are added to.  The
stored 16-bit value lies in [round_T(lo), round_T(hi)] with
    ReLU before the skips (DPT):      lo / hi = relu(zc -/+ bc) + r -/+ ba
    ReLU after the skips (bottleneck): lo / hi = relu(zc + r -/+ (bc + ba))
    no ReLU:                           lo / hi = zc + r -/+ (bc + ba)
whose width never exceeds (K_range + 1 + nres) 2^-23 (Sc + |res| + |res2|), the family's stated bound.  The interval is handed to
gemm_helpers.check_16 as its midpoint and half-width with the identity activation (one fp64 rounding of each end: 1e-16 relative).
out_relu equals, bit for bit, the kernel's OWN stored out with its negative halves cleared (-0 -> +0).

Inputs.  b / ulp(z) = K 2^-23 (S / |z|) 2^11 for fp16: at K = 1152 zero-mean operands (S / |z| ~ 20) would make every interval two-ended.
So x is positive (3 % of it negated; 40 % where relu_in reads it) and every output channel's weights, bias and skips share one sign, drawn
per channel: S / |z| ~ 1.06, half of the pre-activations are negative, and no case has more than half of its intervals two-ended
(asserted).  The weight gradients have fp32 outputs and use zero-mean operands.
"""
import ctypes as C

import numpy as np
import torch
import torch.nn.functional as F

import gemm_helpers as G
from gemm_helpers import Out, round_to, act_range, check_16, check_f32, assert_within, assert_bits_equal, RATIOS, WIDENED, U23, TD, LD  # noqa: F401
from glue_helpers import _bits
from lseg_hip import _lib

EPI_GENERIC, EPI_PAD16, EPI_PART32 = 0, 5, 8
TILE_EDGE = {1: 64, 2: 128, 6: 256}
CONDITIONS = {}              # case name -> {"neg_pre": share, "neg_in": share, "neg_stored": count}: the input conditions, from the reference alone


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _pos(shape, g, lo=0.25):
    return torch.randn(shape, generator=g).abs() + lo


# ---- forward cases ------------------------------------------------------------------------------------------------------------------------------------
def fcase(name, B, H, W, Cin, Cout, dt, exp, k=3, s=1, relu_in=0, relu=0, nres=0, rar=0, out_relu=0, alias=0, tile=0, max_grid=0, nsplit=0, steps=0):
    """exp = (epilogue, tile, most work items of a workgroup) the launcher must choose, at 256 and at 64 CUs."""
    return dict(name=name, B=B, H=H, W=W, Cin=Cin, Cout=Cout, dt=dt, exp=exp, k=k, s=s, relu_in=relu_in, relu=relu, nres=nres, rar=rar,
                out_relu=out_relu, alias=alias, tile=tile, max_grid=max_grid, nsplit=nsplit, steps=steps)


HEADS = ((64, 1, EPI_GENERIC), (128, 1, EPI_PAD16), (128, 2, EPI_PAD16), (256, 6, EPI_PAD16))       # (Cout, tile, epilogue)
S1_MAP = {1: (3, 5, 7), 2: (2, 9, 8), 6: (3, 10, 10)}        # tile -> (B, H, W): M = 105 | 144 | 300, ragged at 64 | 128 | 256, tile rows straddle images


def _geometry_cases():
    cs = []
    for Cout, tile, epi in HEADS:
        for dt in ("bf16", "f16"):
            for Cin in (64, 128):
                B, H, W = S1_MAP[tile]
                cs.append(fcase(f"geo.s1.{H}x{W}.k3.ci{Cin}.co{Cout}.t{tile}.{dt}", B, H, W, Cin, Cout, dt, (epi, tile, 1), tile=tile))
                for H2, W2 in ((7, 5), (6, 8)):
                    for k in (3, 1):
                        cs.append(fcase(f"geo.s2.{H2}x{W2}.k{k}.ci{Cin}.co{Cout}.t{tile}.{dt}", 3, H2, W2, Cin, Cout, dt, (epi, tile, 1), k=k, s=2, tile=tile))
            B, H, W = S1_MAP[tile]
            cs.append(fcase(f"geo.s1.{H}x{W}.k1.ci64.co{Cout}.t{tile}.{dt}", B, H, W, 64, Cout, dt, (epi, tile, 1), k=1, tile=tile))
    for dt in ("bf16", "f16"):
        # max_grid = 8: one workgroup per XCD walks several tiles, the A cursor carries its tap state across a tile boundary
        cs.append(fcase(f"geo.walk.t1.{dt}", 3, 10, 10, 64, 256, dt, (EPI_PAD16, 1, 3), tile=1, max_grid=8))       # 5 x 4 tiles
        cs.append(fcase(f"geo.walk.t2.{dt}", 3, 10, 10, 64, 512, dt, (EPI_PAD16, 2, 2), tile=2, max_grid=8))       # 3 x 4 tiles
        cs.append(fcase(f"geo.walk.t6.{dt}", 6, 10, 10, 64, 768, dt, (EPI_PAD16, 6, 2), tile=6, max_grid=8))       # 3 x 3 tiles
        cs.append(fcase(f"geo.walk.generic.{dt}", 6, 10, 10, 64, 64, dt, (EPI_GENERIC, 1, 2), tile=1, max_grid=8))  # 10 x 1 tiles
    return cs


FORMS = (("plain", {}), ("relu", dict(relu=1)), ("relu_in", dict(relu_in=1, relu=1)), ("res", dict(nres=1)), ("res2", dict(nres=2)),
         ("relu+res2", dict(relu=1, nres=2)), ("rar1", dict(relu=1, nres=1, rar=1)), ("rar2", dict(relu=1, nres=2, rar=1)),
         ("outrelu", dict(out_relu=1)), ("outrelu+res2", dict(out_relu=1, nres=2)), ("alias", dict(nres=1, alias=1)),
         ("alias.rar", dict(relu=1, nres=1, rar=1, alias=1)))


def _epilogue_cases():
    cs = []
    for Cout, tile, epi in HEADS:
        B, H, W = S1_MAP[tile]
        for dt in ("bf16", "f16"):
            for label, kw in FORMS:
                if kw.get("out_relu") and epi != EPI_PAD16:
                    continue                                    # the generic epilogue has no ReLU copy: refused (test_gpu_conv_family, host test)
                cs.append(fcase(f"epi.{label}.co{Cout}.t{tile}.{dt}", B, H, W, 64, Cout, dt, (epi, tile, 1), tile=tile, **kw))
    return cs


SPLITS = ((18, 4, 5), (18, 6, 3), (18, 18, 1), (18, 2, 9))       # (nk, nsplit, split_steps) at Cin = 128: a tap is 2 steps, odd steps begin mid-tap


def _split_cases():
    cs = []
    for tile in (1, 2, 6):
        B, H, W = S1_MAP[tile]
        Cout = 256 if tile == 6 else 128
        for nk, ns, st in SPLITS:
            for dt in ("bf16", "f16"):
                tiles = -(-B * H * W // TILE_EDGE[tile]) * (Cout // TILE_EDGE[tile]) * ns
                cs.append(fcase(f"split.t{tile}.{ns}x{st}.{dt}", B, H, W, 128, Cout, dt, (EPI_PART32, tile, -(-tiles // 8)), tile=tile, max_grid=8,
                                nsplit=ns, steps=st))
    return cs


GEOMETRY, EPILOGUE, SPLIT = _geometry_cases(), _epilogue_cases(), _split_cases()
FORWARD = GEOMETRY + EPILOGUE
assert len({c["name"] for c in FORWARD + SPLIT}) == len(FORWARD + SPLIT)


def ids(cs):
    return [c["name"] for c in cs]


def out_hw(c):
    return (c["H"] - 1) // c["s"] + 1, (c["W"] - 1) // c["s"] + 1


# ---- forward data and reference -------------------------------------------------------------------------------------------------------------------------
_DATA, _REF = {}, {}


def fdata(c):
    """x_pad [B, H+2, W+2, Cin] (border random, non-zero), w4 [Cout, Cin, k, k], W = its tap-major packing [Cout, k k Cin], bias fp32,
    res / res2 [B, Ho+2, Wo+2, Cout] -- from seeds, shared by the cases of one geometry."""
    key = (c["B"], c["H"], c["W"], c["Cin"], c["Cout"], c["k"], c["s"], c["dt"], c["relu_in"])
    if key in _DATA:
        return _DATA[key]
    g = _gen(3000 + sum((i + 1) * 131 ** i * v for i, v in enumerate(key[:7])) % 100003 + (7 if c["dt"] == "f16" else 0) + 13 * c["relu_in"])
    dt, (Ho, Wo) = TD[c["dt"]], out_hw(c)
    K = c["k"] * c["k"] * c["Cin"]
    x = _pos((c["B"], c["H"] + 2, c["W"] + 2, c["Cin"]), g)
    x = torch.where(torch.rand(x.shape, generator=g) < (0.4 if c["relu_in"] else 0.03), -x, x)
    sign = torch.where(torch.rand(c["Cout"], generator=g) < 0.5, -1.0, 1.0)
    sign[:2] = torch.tensor([1.0, -1.0])
    w4 = _pos((c["Cout"], c["Cin"], c["k"], c["k"]), g) * K ** -0.5 * sign[:, None, None, None]
    d = dict(x=x.to(dt), w4=w4.to(dt), bias=(_pos((c["Cout"],), g, 0.0) * 0.5 * sign).float(), sign=sign)
    d["W"] = d["w4"].permute(0, 2, 3, 1).reshape(c["Cout"], K).contiguous()
    for r in ("res", "res2"):
        d[r] = (_pos((c["B"], Ho + 2, Wo + 2, c["Cout"]), g, 0.1) * sign).to(dt)
    _DATA[key] = d
    return d


def conv64(c, d, k0=0, k1=None):
    """(zc, Sc) over the K-range [k0, k1) of the tap-major contraction (whole: with the bias), [B, Ho, Wo, Cout] fp64."""
    key = (id(d), k0, k1)
    if key in _REF:
        return _REF[key]
    x = d["x"].double().permute(0, 3, 1, 2)
    if c["relu_in"]:
        x = x.clamp(min=0)
    if c["k"] == 1:
        x = x[:, :, 1:-1, 1:-1]
    w = d["w4"].double()
    whole = k0 == 0 and k1 is None
    if not whole:                                                 # tap-major K: k = (ky * 3 + kx) * Cin + ci; the range as a mask on the weight
        m = torch.zeros(c["k"] * c["k"] * c["Cin"], dtype=torch.bool)
        m[k0:k1] = True
        w = w * m.reshape(c["k"], c["k"], c["Cin"]).permute(2, 0, 1)[None].double()
    b = d["bias"].double() if whole else None
    z = F.conv2d(x, w, b, stride=c["s"], padding=0).permute(0, 2, 3, 1).contiguous()
    S = F.conv2d(x.abs(), w.abs(), b.abs() if whole else None, stride=c["s"], padding=0).permute(0, 2, 3, 1).contiguous()
    _REF[key] = (z, S)
    return z, S


def _interior(t):
    return t[:, 1:-1, 1:-1]


def finterval(c, d):
    """(lo, hi) fp64 of the stored value before its rounding, [B, Ho, Wo, Cout]; records the case's input conditions."""
    zc, Sc = conv64(c, d)
    K = c["k"] * c["k"] * c["Cin"]
    bc = (K + 1) * U23 * Sc
    r = torch.zeros_like(zc)
    ra = torch.zeros_like(zc)
    for i in range(c["nres"]):
        t = _interior(d[("res", "res2")[i]].double())
        r, ra = r + t, ra + t.abs()
    if c["relu"] and not c["rar"]:
        tlo, thi = (zc - bc).clamp(min=0), (zc + bc).clamp(min=0)
        ba = c["nres"] * U23 * (thi + ra)
        lo, hi, pre = tlo + r - ba, thi + r + ba, zc
    else:
        ba = c["nres"] * U23 * (zc.abs() + bc + ra)
        lo, hi, pre = zc + r - bc - ba, zc + r + bc + ba, zc + r
        if c["relu"]:
            lo, hi = lo.clamp(min=0), hi.clamp(min=0)
    CONDITIONS[c["name"]] = dict(neg_pre=(pre < 0).double().mean().item() if c["relu"] else None,
                                 neg_in=(d["x"].float() < 0).float().mean().item() if c["relu_in"] else None,
                                 neg_stored=int((hi < 0).sum()) if c["out_relu"] else None)
    return lo, hi


def _embed_pad(c, t):
    Ho, Wo = out_hw(c)
    e = torch.zeros(c["B"], Ho + 2, Wo + 2, c["Cout"], dtype=torch.float64)
    e[:, 1:-1, 1:-1] = t
    return e


def fmust(c):
    Ho, Wo = out_hw(c)
    m = torch.zeros(c["B"], Ho + 2, Wo + 2, c["Cout"], dtype=torch.bool)
    m[:, 1:-1, 1:-1] = True
    return m


def make_fouts(c, d, device):
    """out (in place: the written cells hold res) and, when asked for, out_relu: padded maps whose border is guard pattern."""
    m = fmust(c)
    outs = {"out": Out(m.shape, c["dt"], m, device, fill=d["res"] if c["alias"] else None)}
    if c["out_relu"]:
        outs["out_relu"] = Out(m.shape, c["dt"], m, device)
    return outs


def relu_bits(t):
    """A 16-bit tensor with its negative halves cleared: the sign-bit test of the epilogue's ReLU copy (-0 -> +0)."""
    b = _bits(t)
    return torch.where(b < 0, torch.zeros_like(b), b)


def print_ratio16(out, lo, hi, name):
    """Printed, not asserted (the interval is the check): worst |stored - mid| / (half-width + half an ulp of the output type at mid)."""
    m = out.must.cpu()
    got, z, b = out.payload().detach().cpu().double()[m], ((lo + hi) / 2)[m], ((hi - lo) / 2)[m]
    ulp = torch.exp2(torch.floor(torch.log2(z.abs().clamp(min=2.0 ** (-126 if out.dt == "bf16" else -14)))) - (7 if out.dt == "bf16" else 10))
    r = ((got - z).abs() / (b + ulp / 2)).max().item()
    RATIOS[name] = r
    print(f"conv-ratio {name}: worst err / (b + ulp/2) = {r:.4f}, two-ended intervals {100 * WIDENED[name]:.3f} %")


def check_forward(c, d, outs, who=""):
    lo, hi = finterval(c, d)
    lo, hi = _embed_pad(c, lo), _embed_pad(c, hi)
    name = who + c["name"]
    check_16(outs["out"], (lo + hi) / 2, (hi - lo) / 2, G.ACT_NONE, name)
    print_ratio16(outs["out"], lo, hi, name)
    assert WIDENED[name] <= 0.5, f"{name}: {100 * WIDENED[name]:.1f} % of the intervals are two-ended (input condition: at most half)"
    if c["out_relu"]:
        got = outs["out_relu"].check(name + ".out_relu")
        m = outs["out"].must.cpu()
        want = relu_bits(outs["out"].payload())
        g = _bits(got)
        bad = ((g != want) & m).nonzero()
        assert not bad.numel(), f"{name}.out_relu: {bad.shape[0]} cells differ bitwise from the stored out with its negative halves cleared, first at {bad[0].tolist()}"


# ---- split-K slabs ------------------------------------------------------------------------------------------------------------------------------------------
def split_ref(c, d):
    """slabs [ns + 1][M][Cout] (one more than the launch owns): z, bound, must."""
    Ho, Wo = out_hw(c)
    M, N, ns, st = c["B"] * Ho * Wo, c["Cout"], c["nsplit"], c["steps"]
    K = 9 * c["Cin"]
    shape = (ns + 1, M, N)
    z, b = torch.zeros(shape, dtype=torch.float64), torch.zeros(shape, dtype=torch.float64)
    must = torch.zeros(shape, dtype=torch.bool)
    must[:ns] = True
    for s in range(ns):
        k0, k1 = 64 * s * st, min(64 * (s + 1) * st, K)
        zs, Ss = conv64(c, d, k0, k1)
        z[s], b[s] = zs.reshape(M, N), (k1 - k0 + 1) * U23 * Ss.reshape(M, N)
    return shape, must, z, b


def make_souts(c, d, device):
    shape, must, _, _ = split_ref(c, d)
    return {"out": Out(shape, "f32", must, device)}


def check_split(c, d, outs, who=""):
    shape, must, z, b = split_ref(c, d)
    check_f32(outs["out"], z, b, who + c["name"])


# ---- conv_reduce_pad ----------------------------------------------------------------------------------------------------------------------------------------
RFORMS = (("plain", {}), ("relu", dict(relu=1)), ("res", dict(nres=1)), ("res2", dict(nres=2)), ("relu+res2", dict(relu=1, nres=2)),
          ("rar1", dict(relu=1, nres=1, rar=1)), ("rar2", dict(relu=1, nres=2, rar=1)), ("outrelu", dict(out_relu=1)),
          ("outrelu+res2", dict(out_relu=1, nres=2)), ("alias", dict(nres=1, alias=1)), ("nobias", dict(bias=0)))


def _reduce_cases():
    cs = []
    for ns, Cc in ((ns, Cc) for ns in (2, 3, 8) for Cc in (8, 64, 256)):
        for dt in ("bf16", "f16"):
            for label, kw in RFORMS:
                c = dict(name=f"reduce.{label}.ns{ns}.C{Cc}.{dt}", B=2, Ho=3, Wo=5, C=Cc, ns=ns, dt=dt, relu=0, nres=0, rar=0, out_relu=0, alias=0, bias=1)
                c.update(kw)
                cs.append(c)
    return cs


REDUCE = _reduce_cases()


def rdata(c):
    key = ("r", c["ns"], c["C"], c["dt"])
    if key in _DATA:
        return _DATA[key]
    g = _gen(4000 + 17 * c["ns"] + c["C"] + (7 if c["dt"] == "f16" else 0))
    M = c["B"] * c["Ho"] * c["Wo"]
    sign = torch.where(torch.rand(c["C"], generator=g) < 0.5, -1.0, 1.0)
    sign[:2] = torch.tensor([1.0, -1.0])
    d = dict(part=(_pos((c["ns"], M + 1, c["C"]), g) * sign).float(), bias=(_pos((c["C"],), g) * sign).float())      # stride = (M + 1) C: a row of slack per slab
    for r in ("res", "res2"):
        d[r] = (_pos((c["B"], c["Ho"] + 2, c["Wo"] + 2, c["C"]), g, 0.1) * sign).to(TD[c["dt"]])
    _DATA[key] = d
    return d


def rinterval(c, d):
    M = c["B"] * c["Ho"] * c["Wo"]
    p = d["part"].double()[:, :M].reshape(c["ns"], c["B"], c["Ho"], c["Wo"], c["C"])
    zc, Sc = p.sum(0), p.abs().sum(0)
    if c["bias"]:
        zc, Sc = zc + d["bias"].double(), Sc + d["bias"].double().abs()
    bc = c["ns"] * U23 * Sc                                       # bias + ns slabs: ns additions
    r, ra = torch.zeros_like(zc), torch.zeros_like(zc)
    for i in range(c["nres"]):
        t = _interior(d[("res", "res2")[i]].double())
        r, ra = r + t, ra + t.abs()
    if c["relu"] and not c["rar"]:
        tlo, thi = (zc - bc).clamp(min=0), (zc + bc).clamp(min=0)
        ba = c["nres"] * U23 * (thi + ra)
        lo, hi, pre = tlo + r - ba, thi + r + ba, zc
    else:
        ba = c["nres"] * U23 * (zc.abs() + bc + ra)
        lo, hi, pre = zc + r - bc - ba, zc + r + bc + ba, zc + r
        if c["relu"]:
            lo, hi = lo.clamp(min=0), hi.clamp(min=0)
    CONDITIONS[c["name"]] = dict(neg_pre=(pre < 0).double().mean().item() if c["relu"] else None, neg_in=None,
                                 neg_stored=int((hi < 0).sum()) if c["out_relu"] else None)
    return lo, hi


def rmust(c):
    m = torch.zeros(c["B"], c["Ho"] + 2, c["Wo"] + 2, c["C"], dtype=torch.bool)
    m[:, 1:-1, 1:-1] = True
    return m


def make_routs(c, d, device):
    m = rmust(c)
    outs = {"out": Out(m.shape, c["dt"], m, device, fill=d["res"] if c["alias"] else None)}
    if c["out_relu"]:
        outs["out_relu"] = Out(m.shape, c["dt"], m, device)
    return outs


def check_reduce(c, d, outs, who=""):
    lo, hi = rinterval(c, d)
    e = lambda t: _embed_pad(dict(B=c["B"], H=c["Ho"], W=c["Wo"], s=1, Cout=c["C"]), t)
    lo, hi = e(lo), e(hi)
    name = who + c["name"]
    check_16(outs["out"], (lo + hi) / 2, (hi - lo) / 2, G.ACT_NONE, name)
    print_ratio16(outs["out"], lo, hi, name)
    assert WIDENED[name] <= 0.5, f"{name}: {100 * WIDENED[name]:.1f} % of the intervals are two-ended"
    if c["out_relu"]:
        got = outs["out_relu"].check(name + ".out_relu")
        bad = ((_bits(got) != relu_bits(outs["out"].payload())) & outs["out"].must.cpu()).nonzero()
        assert not bad.numel(), f"{name}.out_relu: {bad.shape[0]} cells differ bitwise from the stored out with its negative halves cleared"


# ---- weight gradients ---------------------------------------------------------------------------------------------------------------------------------------
def _wgrad_cases():
    cs = []
    for Cin, Cout in ((128, 64), (256, 192)):
        for B, H, W, slabs, tight in ((1, 6, 5, 1, 0), (2, 22, 22, 2, 0), (2, 22, 22, 1, 1)):
            for relu_x in (0, 1):
                for dt in ("bf16", "f16"):
                    cs.append(dict(name=f"wgrad.ci{Cin}.co{Cout}.B{B}.{H}x{W}.{'ws1' if tight else 'ws'}.relu{relu_x}.{dt}", B=B, H=H, W=W, Cin=Cin,
                                   Cout=Cout, relu_x=relu_x, dt=dt, slabs=slabs, tight=tight))
    return cs


def _linear_wgrad_cases():
    cs = []
    for M in (37, 64, 130):
        for cols in (128, 384):
            for acc in (0, 1):
                for dt in ("bf16", "f16"):
                    cs.append(dict(name=f"wlin.M{M}.cols{cols}.acc{acc}.{dt}", M=M, rows=40, ldy=48, cols=cols, ldx=cols + 8, acc=acc, dt=dt))
    return cs


WGRAD, WLIN = _wgrad_cases(), _linear_wgrad_cases()


def wdata(c):
    key = ("w", c["B"], c["H"], c["W"], c["Cin"], c["Cout"], c["dt"])
    if key in _DATA:
        return _DATA[key]
    g = _gen(5000 + c["B"] + 3 * c["H"] + c["Cin"] + c["Cout"] + (7 if c["dt"] == "f16" else 0))
    dt = TD[c["dt"]]
    x = torch.randn((c["B"], c["H"] + 2, c["W"] + 2, c["Cin"]), generator=g)            # border random: the tap shifts read it
    dy = torch.zeros(c["B"], c["H"] + 2, c["W"] + 2, c["Cout"])
    dy[:, 1:-1, 1:-1] = torch.randn((c["B"], c["H"], c["W"], c["Cout"]), generator=g)      # zero border: the contract
    d = dict(x=x.to(dt), dy=dy.to(dt))
    _DATA[key] = d
    return d


def wgrad_ref(c, d):
    """dW [Cout, 9, Cin] tap-major fp64 by autograd of conv2d over the padded map; S from the same gradient of the absolute values."""
    key = (id(d), c["relu_x"])
    if key in _REF:
        return _REF[key]
    x = d["x"].double().permute(0, 3, 1, 2)
    if c["relu_x"]:
        x = x.clamp(min=0)
    dy = _interior(d["dy"].double()).permute(0, 3, 1, 2)
    w = torch.zeros(c["Cout"], c["Cin"], 3, 3, dtype=torch.float64, requires_grad=True)
    (gw,) = torch.autograd.grad((F.conv2d(x, w, None, stride=1, padding=0) * dy).sum(), w)
    S = torch.nn.grad.conv2d_weight(x.abs(), w.shape, dy.abs(), stride=1, padding=0)
    shape = (c["Cout"], 9, c["Cin"])
    _REF[key] = (gw.permute(0, 2, 3, 1).reshape(shape), S.permute(0, 2, 3, 1).reshape(shape))
    return _REF[key]


POISON_ROWS, POISON = 128, 3.0


def poisoned(t, device):
    """A K-major operand (rows of its last dimension) on `device` with POISON_ROWS rows of the finite non-zero value POISON before and
    behind it: more than the 63 rows to the next multiple of 64 plus the largest tap shift (W + 3 <= 27 rows).  A kernel that took the
    rows at or beyond k_valid, or the shifted rows below 0, as data adds 9 per such row to dW -- whatever else the allocator holds.
    Returns (the whole buffer, the view of t inside it)."""
    ld = t.shape[-1]
    buf = torch.full((2 * POISON_ROWS * ld + t.numel(),), POISON, dtype=t.dtype, device=device)
    view = buf[POISON_ROWS * ld:POISON_ROWS * ld + t.numel()].view(t.shape)
    view.copy_(t)
    return buf, view


def wgrad_ws_floats(c):
    return c["Cout"] * 9 * c["Cin"] * (1 if c["tight"] else 4)


def check_wgrad(c, d, out, ns, who=""):
    z, S = wgrad_ref(c, d)
    Mp = c["B"] * (c["H"] + 2) * (c["W"] + 2)
    assert ns == c["slabs"], f"{c['name']}: {ns} slabs, written for {c['slabs']}"
    check_f32(out, z, (Mp + ns) * U23 * S, who + c["name"])


def ldata(c):
    key = ("l", c["M"], c["cols"], c["dt"])
    if key in _DATA:
        return _DATA[key]
    g = _gen(6000 + c["M"] + c["cols"] + (7 if c["dt"] == "f16" else 0))
    d = dict(dy=torch.randn((c["M"], c["ldy"]), generator=g).to(TD[c["dt"]]), x=torch.randn((c["M"], c["ldx"]), generator=g).to(TD[c["dt"]]),
             dw0=torch.randn((c["rows"], c["cols"]), generator=g))
    _DATA[key] = d
    return d


def check_wlin(c, d, out, who=""):
    dy, x = d["dy"].double()[:, :c["rows"]], d["x"].double()[:, :c["cols"]]
    z, S = dy.T @ x, dy.abs().T @ x.abs()
    if c["acc"]:
        z, S = z + d["dw0"].double(), S + d["dw0"].double().abs()
    check_f32(out, z, (c["M"] + 1 + c["acc"]) * U23 * S, who + c["name"])


# ---- packers ------------------------------------------------------------------------------------------------------------------------------------------------
DGRAD_PACK = [dict(name=f"dgradpack.co{co}.ci{ci}.{dt}", Co=co, Ci=ci, dt=dt) for co, ci in ((64, 128), (192, 64)) for dt in ("bf16", "f16")]
PACK3 = [dict(name=f"pack3.{'bn' if bn else 'nobn'}.{'cb' if cb else 'nocb'}.ci{ci}-{cip}.{dt}", Co=24, Ci=ci, Cip=cip, bn=bn, cb=cb, dt=dt)
         for bn in (0, 1) for cb in (0, 1) for ci, cip in ((3, 64), (64, 64)) for dt in ("f32", "bf16", "f16")]
PACK1 = [dict(name=f"pack1.{'bn' if bn else 'nobn'}.{dt}", Co=40, Ci=72, bn=bn, dt=dt) for bn in (0, 1) for dt in ("bf16", "f16")]
BN_EPS = 1e-5


def pdata(c):
    g = _gen(7000 + c["Co"] + c["Ci"])
    k = 3 if "Cip" in c else 1
    return dict(w=torch.randn((c["Co"], c["Ci"], k, k), generator=g), bn_w=_pos((c["Co"],), g), bn_b=torch.randn(c["Co"], generator=g),
                bn_m=torch.randn(c["Co"], generator=g), bn_v=_pos((c["Co"],), g, 0.05), cb=torch.randn(c["Co"], generator=g))


def dgrad_pack_data(c):
    w4 = torch.randn((c["Co"], c["Ci"], 3, 3), generator=_gen(7100 + c["Co"])).to(TD[c["dt"]])
    return dict(w4=w4, wp=w4.permute(0, 2, 3, 1).contiguous())      # [Co, 9, Ci] tap-major


def dgrad_pack_ref(d):
    """The transposed conv's weight: taps flipped, channels swapped, packed tap-major for a conv with Cin' = Co: [Ci, 9, Co]."""
    return d["w4"].flip(2, 3).transpose(0, 1).permute(0, 2, 3, 1).contiguous()


def pack_ref(c, d):
    """(v [Co, k, k, Ci] fp64, bv its bound, bias fp64, its bound).  The fold is s = bn_w / sqrt(bn_v + eps) in fp32 -- one addition, one
    reciprocal square root (taken as 2 ulp), one multiply: 3 x 2^-23 relative -- then ONE fp32 multiply w s and one rounding to the output
    type: v within 4 x 2^-23 |w s|, exact without BatchNorm; the bias conv_bias s + bn_b - bn_m s in fp32: 6 x 2^-23 of its absolute sum."""
    w = d["w"].double()
    if c["bn"]:
        s = d["bn_w"].double() / (d["bn_v"].double() + BN_EPS).sqrt()
    else:
        s = torch.ones(c["Co"], dtype=torch.float64)
    v = (w * s[:, None, None, None]).permute(0, 2, 3, 1).contiguous()
    bv = (4 * U23 * v.abs()) if c["bn"] else torch.zeros_like(v)
    cb = d["cb"].double() * s if c.get("cb") else torch.zeros(c["Co"], dtype=torch.float64)
    bias, babs = cb.clone(), cb.abs()
    if c["bn"]:
        bias = bias + d["bn_b"].double() - d["bn_m"].double() * s
        babs = babs + d["bn_b"].double().abs() + (d["bn_m"].double() * s).abs()
    return v, bv, bias, 6 * U23 * babs


def make_pouts(c, device):
    """wp [Co, taps, Cip]: channels ci < Ci must be written; the pad channels hold the caller's ZEROS and must keep them.  bias [Co]."""
    taps, cip = (9, c["Cip"]) if "Cip" in c else (1, c["Ci"])
    must = torch.zeros(c["Co"], taps, cip, dtype=torch.bool)
    must[..., :c["Ci"]] = True
    return {"wp": Out(must.shape, c["dt"], must, device, outside=0), "bias": Out((c["Co"],), "f32", torch.ones(c["Co"], dtype=torch.bool), device)}


def pack_has_bias(c):
    return bool(c["bn"] or c.get("cb")) or "Cip" not in c


def check_pack(c, d, outs, who=""):
    v, bv, bias, bb = pack_ref(c, d)
    taps = 9 if "Cip" in c else 1
    name = who + c["name"]
    z = torch.zeros(outs["wp"].shape, dtype=torch.float64)
    b = torch.zeros_like(z)
    z[..., :c["Ci"]], b[..., :c["Ci"]] = v.reshape(c["Co"], taps, c["Ci"]), bv.reshape(c["Co"], taps, c["Ci"])
    if c["dt"] == "f32":
        check_f32(outs["wp"], z, b + U23 / 2 * z.abs(), name)           # the store is the fp32 product itself: its own rounding
    else:
        check_16(outs["wp"], z, b, G.ACT_NONE, name)
        print_ratio16(outs["wp"], z - b, z + b, name)
        assert WIDENED[name] <= 0.5, f"{name}: {100 * WIDENED[name]:.1f} % of the intervals are two-ended (input condition: at most half)"
    pads =outs["wp"].payload()[~outs["wp"].must]
    assert (_bits(pads) == 0).all(), f"{name}: a pad channel is not zero"
    if pack_has_bias(c):
        check_f32(outs["bias"], bias, bb, name + ".bias")
    else:
        outs["bias"].untouched(name + ".bias")


# ---- the C struct and the plan ----------------------------------------------------------------------------------------------------------------------------
FAKE = 0x7F0000000000


def struct_of(c, ptrs=None):
    p = ptrs or {k: FAKE + 0x1000000 * i for i, k in enumerate(("x", "W", "bias", "res", "res2", "out", "out_relu"))}
    g = _lib.LSegConvCase()
    g.inp, g.w, g.out = p["x"], p["W"], p["out"]
    g.B, g.H, g.W, g.Cin, g.Cout, g.ksize, g.stride, g.dtype = c["B"], c["H"], c["W"], c["Cin"], c["Cout"], c["k"], c["s"], LD[c["dt"]]
    g.tile, g.max_grid = c["tile"], c["max_grid"]
    if c["nsplit"] > 1:
        Ho, Wo = out_hw(c)
        g.nsplit, g.split_steps, g.c_split_stride = c["nsplit"], c["steps"], c["B"] * Ho * Wo * c["Cout"]
        return g
    g.bias = p["bias"]
    g.relu_in, g.relu_out, g.relu_after_res = c["relu_in"], c["relu"], c["rar"]
    if c["nres"] >= 1:
        g.residual = p["out"] if c["alias"] else p["res"]
    if c["nres"] >= 2:
        g.residual2 = p["res2"]
    if c["out_relu"]:
        g.out_relu = p["out_relu"]
    return g


def plan(lib, g, cus):
    out4 = (C.c_int * 4)()
    r = lib.lseg_op_conv_ex_plan(C.byref(g), cus, C.byref(out4))
    return r, tuple(out4)


def assert_plan(lib, c, g, cus):
    r, p = plan(lib, g, cus)
    assert r == 0, f"{c['name']}: the plan was refused ({r}): {lib.lseg_last_error(None)}"
    assert (p[0], p[1], p[3]) == tuple(c["exp"]), f"{c['name']} at {cus} CUs: runs (epilogue, tile, items) = {(p[0], p[1], p[3])}, written for {c['exp']}"
    return p


# ---- fp32 emulations (host self-check) and their wrong variants ------------------------------------------------------------------------------------
def _emu_conv(c, d, wrong=None, k0=0, k1=None):
    """fp32, ascending k (tap by tap, channel chunks of 64 inside a tap), from the kernel's index arithmetic: acc [M, Cout]."""
    B, H, W, Cin, Cout, k, s = c["B"], c["H"], c["W"], c["Cin"], c["Cout"], c["k"], c["s"]
    Ho, Wo = out_hw(c)
    x = d["x"].float()
    if c["relu_in"]:
        x = x.clamp(min=0)
    if wrong == "border-as-zero":
        x = x.clone()
        x[:, 0], x[:, -1], x[:, :, 0], x[:, :, -1] = 0, 0, 0, 0
    Wm = d["W"].float()
    K = k * k * Cin
    k1 = K if k1 is None else k1
    m = torch.arange(B * Ho * Wo)
    b, y, xx = m // (Ho * Wo), (m % (Ho * Wo)) // Wo, m % Wo
    if wrong == "image-base-of-tile":                                # every row of a tile takes the image of the tile's first row
        e = TILE_EDGE[c["exp"][1]]
        b = b[(m // e) * e]
    acc = torch.zeros(B * Ho * Wo, Cout)
    for kk in range(k0, k1, 64):
        tap, c0 = kk // Cin, kk % Cin
        ky, kx = (1, 1) if k == 1 else (tap // 3, tap % 3)
        if wrong == "kykx":
            ky, kx = kx, ky
        o = 1 if (wrong == "stride-origin" and s == 2) else 0
        rows = x[b, (y * s + ky + o).clamp(max=H + 1), (xx * s + kx + o).clamp(max=W + 1), c0:c0 + 64]
        acc = acc + rows @ Wm[:, kk:kk + 64].T
    return acc


def _emu_epilogue(c, v, bias, res, res2, dt, wrong=None):
    """v [.., C] fp32 accumulators -> (stored 16-bit, ReLU copy) in the kernel's order."""
    rar = c["rar"]
    if wrong == "relu-side" and c["relu"] and c["nres"]:
        rar = 1 - rar
    if bias is not None:
        v = v + bias
    if c["relu"] and not rar:
        v = v.clamp(min=0)
    pre = v
    if c["nres"] >= 1:
        v = v + res.float()
    if c["nres"] >= 2 and wrong != "drop-res2":
        v = v + res2.float()
    if c["relu"] and rar:
        v = v.clamp(min=0)
    st = v.to(dt)
    if wrong == "outrelu-before-skips":
        cp = pre.clamp(min=0).to(dt)
    elif wrong == "outrelu-keeps-minus-zero":
        cp = torch.where(st.float() < 0, torch.tensor(-0.0).to(dt), st)
    else:
        cp = relu_bits(st).view(dt)
    return st, cp


def emulate_forward(c, d, wrong=None):
    outs = make_fouts(c, d, "cpu")
    Ho, Wo = out_hw(c)
    acc = _emu_conv(c, d, wrong).reshape(c["B"], Ho, Wo, c["Cout"])
    st, cp = _emu_epilogue(c, acc, d["bias"], _interior(d["res"]), _interior(d["res2"]), TD[c["dt"]], wrong)
    outs["out"].payload()[:, 1:-1, 1:-1] = st
    if wrong == "zero-border":
        p = outs["out"].payload()
        p[:, 0], p[:, -1], p[:, :, 0], p[:, :, -1] = 0, 0, 0, 0
    if c["out_relu"]:
        outs["out_relu"].payload()[:, 1:-1, 1:-1] = cp
    return outs


def emulate_split(c, d, wrong=None):
    outs = make_souts(c, d, "cpu")
    K, st = 9 * c["Cin"], c["steps"]
    for s in range(c["nsplit"]):
        if wrong == "drop-range" and s == 1:
            continue
        k0, k1 = 64 * s * st, min(64 * (s + 1) * st, K)
        if wrong == "range-early" and s == 1:
            k0 -= 64
        outs["out"].payload()[s] = _emu_conv(c, d, None, k0, k1)
    return outs


def emulate_reduce(c, d, wrong=None):
    outs = make_routs(c, d, "cpu")
    M = c["B"] * c["Ho"] * c["Wo"]
    v = d["bias"].clone().expand(M, c["C"]).clone() if c["bias"] else torch.zeros(M, c["C"])
    for s in range(c["ns"]):
        if wrong == "drop-range" and s == c["ns"] - 1:
            continue
        v = v + d["part"][s, :M]
    v = v.reshape(c["B"], c["Ho"], c["Wo"], c["C"])
    st, cp = _emu_epilogue(c, v, None, _interior(d["res"]), _interior(d["res2"]), TD[c["dt"]], wrong)
    outs["out"].payload()[:, 1:-1, 1:-1] = st
    if wrong == "zero-border":
        p = outs["out"].payload()
        p[:, 0], p[:, -1], p[:, :, 0], p[:, :, -1] = 0, 0, 0, 0
    if c["out_relu"]:
        outs["out_relu"].payload()[:, 1:-1, 1:-1] = cp
    return outs


def wgrad_out(c, device):
    shape = (c["Cout"], 9, c["Cin"])
    return Out(shape, "f32", torch.ones(shape, dtype=torch.bool), device)


def emulate_wgrad(c, d, wrong=None):
    """dW[co, tap, ci] = sum_k dy[k, co] x[k + (tap / 3 - 1) Wp + tap % 3 - 1, ci] over the padded pixels k < k_valid, rows outside
    [0, k_valid) zero: fp32, one product per tap."""
    Mp, Wp = c["B"] * (c["H"] + 2) * (c["W"] + 2), c["W"] + 2
    x, dy = d["x"].float().reshape(Mp, c["Cin"]), d["dy"].float().reshape(Mp, c["Cout"])
    if c["relu_x"] and wrong != "relu_x-ignored":
        x = x.clamp(min=0)
    Kp = -(-Mp // 64) * 64
    if wrong == "tail-as-data":                                       # rows k_valid .. Kp - 1 of the last K-step taken from the poison behind the maps
        x, dy, Mp = torch.cat([x, torch.full((Kp - Mp, c["Cin"]), POISON)]), torch.cat([dy, torch.full((Kp - Mp, c["Cout"]), POISON)]), Kp
    out = wgrad_out(c, "cpu")
    for tap in range(9):
        sh = (tap // 3 - 1) * Wp + (tap % 3 - 1)
        if wrong == "shift-sign":
            sh = -sh
        idx = torch.arange(Mp) + sh
        ok = (idx >= 0) & (idx < Mp)
        xs = torch.where(ok[:, None], x[idx.clamp(0, Mp - 1)], torch.zeros(()))
        out.payload()[:, tap] = dy.T @ xs
    return out


def wlin_out(c, d, device):
    shape = (c["rows"], c["cols"])
    return Out(shape, "f32", torch.ones(shape, dtype=torch.bool), device, fill=d["dw0"])


def emulate_wlin(c, d, wrong=None):
    out = wlin_out(c, d, "cpu")
    dy, x = d["dy"].float()[:, :c["rows"]], d["x"].float()[:, :c["cols"]]
    if wrong == "tail-as-data" and c["M"] % 64:
        dy, x = torch.cat([dy, torch.full((1, c["rows"]), POISON)]), torch.cat([x, torch.full((1, c["cols"]), POISON)])
    v = dy.T @ x
    out.payload()[:] = v + d["dw0"] if (c["acc"] and wrong != "no-accumulate") else v
    return out


def emulate_pack(c, d, wrong=None):
    outs = make_pouts(c, "cpu")
    taps = 9 if "Cip" in c else 1
    if c["bn"]:
        s = d["bn_w"] * torch.rsqrt(d["bn_v"] + torch.tensor(BN_EPS))
    else:
        s = torch.ones(c["Co"])
    v = (d["w"] * s[:, None, None, None]).permute(0, 2, 3, 1).reshape(c["Co"], taps, c["Ci"])
    outs["wp"].payload()[..., :c["Ci"]] = v.to(TD[c["dt"]])
    if wrong == "pad-channel" and outs["wp"].shape[-1] > c["Ci"]:
        outs["wp"].payload()[0, 0, c["Ci"]] = 1.0
    if pack_has_bias(c):
        b = d["cb"] * s if c.get("cb") else torch.zeros(c["Co"])
        if c["bn"]:
            b = b + (d["bn_b"] - d["bn_m"] * s)
        outs["bias"].payload()[:] = b
    return outs
