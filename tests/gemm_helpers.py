"""References, counted bounds, guarded buffers and case tables for the GEMM family (csrc/gemm.hip through lseg_op_gemm_ex).

Reference.  fp64 torch on the operands after their rounding to the operand type, written from the PyTorch operation each form stands for
(nn.Linear; timm's qkv reshape / permute; F.conv_transpose2d; cat(cls, patches) + pos), never from the kernel's index arithmetic.

Bound, counted.  A product of two bf16 or two fp16 values is exact in fp32, so only additions round.  With
S[m, n] = sum_k |A[m, k]| |W[n, k]| + |bias[n]| + |res[m, n]| (fp64) every summation order whose additions are faithfully rounded stays
within b[m, n] = (K_range + 3) 2^-23 S[m, n] of the fp64 value, K_range being the K this work item contracts over.  fp32 outputs are held
to |out - ref| <= b.  16-bit outputs are held to an INTERVAL: the stored value lies between round_T of the two ends of the epilogue
function's range over [z - b, z + b] (identity and ReLU are monotone; GELU has its minimum at z = -0.7518, which is included when the
interval straddles it, and is widened by gelu_fast's own stated error, 4.6e-7 absolute + 2^-23 |ref|, and by its stated -3e-10 |x| tail
below -6.2225).  round_T is one rounding from fp64 (numpy for fp16, an explicit round-half-even to 8 significant bits for bf16).
Every element of every case is checked.

Guards.  An output lives in a flat buffer [PRE | payload | POST] filled with a NaN-free pattern that differs from cell to cell; the cells a
form must write are pre-filled with NaN (or with the residual, in place).  After a run every such cell is finite and every other cell
-- pad rows, qkv pad tokens, the pixel-shuffle border, cls rows, slabs beyond nsplit, PRE and POST -- holds its pattern bit for bit.
The builders fix ldc = N for the row-major forms, so there are no guard COLUMNS beside a row: a stray store to a column n >= N lands in
the next row's cells, which must be written; it is seen only through that cell's value (when the stray store comes last) or, behind the
last row, through the pad rows.  The qkv pad tokens, the pixel-shuffle border and the cls rows are guard cells between written ones.

tests/test_gemm_family_host.py feeds plain fp32 emulations and wrong variants through the same functions; tests/test_gpu_gemm_family.py
feeds the kernels' outputs.
"""
import ctypes as C
import math

import numpy as np
import torch
import torch.nn.functional as F

from glue_helpers import RATIOS, _bits, assert_bits_equal, assert_within  # noqa: F401  (re-exported to the tests)
from lseg_hip import _lib

U23 = 2.0 ** -23
GELU_ABS = 4.6e-7            # gemm.hip, comment above gelu_fast: "GELU error <= 4.6e-7 absolute in fp32 evaluation"
GELU_TAIL = 3e-10            # ... "for very negative x the result is -3e-10 |x| instead of -> 0"
GELU_KNEE = 6.222539901733398
GELU_MIN_X = -0.7517915246935645      # argmin of x Phi(x): Phi(x) + x phi(x) = 0
QSCALE = float(np.float32(0.125 * math.log2(math.e)))
EPI = dict(GENERIC=0, LIN16=1, GELU=2, RES32=3, QKV16=4, F16=6, PIX16=7, PART32=8, LIN32=11)
TD = {"bf16": torch.bfloat16, "f16": torch.float16, "f32": torch.float32}
LD = {"bf16": _lib.LSEG_BF16, "f16": _lib.LSEG_F16, "f32": _lib.LSEG_F32}
ACT_NONE, ACT_GELU, ACT_RELU = 0, 1, 3
WIDENED = {}                 # case name -> share of 16-bit outputs whose interval has two different ends
PRE = 256                    # guard elements on each side of a payload (a multiple of 16 bytes for every type)


# ---- rounding an fp64 value ONCE to a 16-bit type ---------------------------------------------------------------------------------------------
def round_to(x64, dt):
    """fp64 -> the nearest value of dt (ties to even), returned in fp64; +-inf past the largest finite value."""
    x = x64.detach().double().contiguous().numpy()
    if dt == "f16":
        with np.errstate(over="ignore"):
            return torch.from_numpy(x.astype(np.float16).astype(np.float64))
    assert dt == "bf16"
    m, e = np.frexp(x)                                          # x = m 2^e, 0.5 <= |m| < 1
    q = np.maximum(e - 8, -133).astype(np.int64)                # 8 significant bits; fixed quantum 2^-133 in the subnormal range
    r = np.ldexp(np.rint(np.ldexp(x, -q)), q)                   # np.rint: half to even
    r = np.where(np.abs(r) >= 2.0 ** 128, np.copysign(np.inf, r), r)
    r = np.where(np.isfinite(x), r, x)
    return torch.from_numpy(r)


def gelu64(x):
    return x * 0.5 * torch.special.erfc(-x / math.sqrt(2.0))


def act_range(lo, hi, act):
    """Range of the epilogue function over [lo, hi] (fp64, element-wise)."""
    if act == ACT_NONE:
        return lo, hi
    if act == ACT_RELU:
        return lo.clamp(min=0), hi.clamp(min=0)
    glo, ghi = gelu64(lo), gelu64(hi)
    rlo, rhi = torch.minimum(glo, ghi), torch.maximum(glo, ghi)
    straddle = (lo < GELU_MIN_X) & (hi > GELU_MIN_X)
    rlo = torch.where(straddle, torch.full_like(rlo, float(gelu64(torch.tensor(GELU_MIN_X, dtype=torch.float64)))), rlo)
    slack = GELU_ABS + U23 * torch.maximum(glo.abs(), ghi.abs())
    tail = torch.where(lo < -GELU_KNEE, GELU_TAIL * lo.abs() * (1 + U23), torch.zeros_like(lo))
    return rlo - slack - tail, rhi + slack


# ---- guarded output buffers -------------------------------------------------------------------------------------------------------------------
def _pattern(n, dtype, device):
    i = torch.arange(n, device=device)
    if dtype == torch.float32:
        return (1000.0 + (i % 251).float()).contiguous()
    return (0x4B00 + (i % 97)).to(torch.int16).view(dtype)      # 14 .. 17 in fp16, 8.4e6 .. 1.2e7 in bf16: finite in both


class Out:
    """[PRE | coff | payload | POST]; `must` (bool, payload-shaped) marks the cells that have to be written.  fill: None = NaN, a number,
    or a payload-shaped tensor (the residual of an in-place launch).  outside: None = the payload cells outside `must` hold the guard
    pattern, a number = they hold that value (a caller's zeros); either way they must come back bit for bit."""

    def __init__(self, shape, dt, must, device="cpu", coff=0, fill=None, outside=None):
        self.shape, self.dt, self.coff = tuple(shape), dt, coff
        self.n = int(np.prod(shape))
        self.flat = _pattern(PRE + coff + self.n + PRE, TD[dt], device)
        self.must = must.to(device)
        assert tuple(must.shape) == self.shape
        pay = self.payload()
        if outside is not None:
            pay[~self.must] = outside
        if fill is None:
            pay[self.must] = float("nan")
        elif torch.is_tensor(fill):
            pay[self.must] = fill.to(device=device, dtype=TD[dt])[self.must]
        else:
            pay[self.must] = fill
        self.before = self.flat.clone()

    def payload(self):
        return self.flat[PRE + self.coff:PRE + self.coff + self.n].view(self.shape)

    def ptr(self):
        return self.payload().data_ptr()

    def check(self, name):
        """Every cell outside `must` holds its pattern bit for bit; every cell inside is finite."""
        a, b = _bits(self.flat), _bits(self.before)
        keep = torch.ones(a.numel(), dtype=torch.bool)
        keep[PRE + self.coff:PRE + self.coff + self.n] = ~self.must.cpu().reshape(-1)
        bad = ((a != b) & keep).nonzero()
        if bad.numel():
            i = int(bad[0]) - PRE - self.coff
            where = list(np.unravel_index(i, self.shape)) if 0 <= i < self.n else f"guard word {int(bad[0])}"
            raise AssertionError(f"{name}: {bad.shape[0]} cells outside the output were written, first at {where}")
        pay = self.payload().detach().cpu()
        holes = (~torch.isfinite(pay.float())) & self.must.cpu()
        assert not holes.any(), f"{name}: {int(holes.sum())} output cells were not written (or are not finite), first at {holes.nonzero()[0].tolist()}"
        return pay

    def untouched(self, name):
        assert torch.equal(_bits(self.flat), _bits(self.before)), f"{name}: a refused call wrote to its output"


# ---- comparisons ----------------------------------------------------------------------------------------------------------------------------------
def check_f32(out, ref, bound, name):
    pay = out.check(name)
    m = out.must.cpu()
    return assert_within(pay[m], ref[m], bound[m], name)


def check_16(out, z, bound, act, name, scale=None):
    """The stored 16-bit values against the interval [round_T(f_lo), round_T(f_hi)], f over [z - b, z + b] (times `scale`, with the
    product's own fp32 rounding, for the pre-scaled q)."""
    pay = out.check(name)
    m = out.must.cpu()
    got, z, b = pay[m].double(), z[m], bound[m]
    lo, hi = act_range(z - b, z + b, act)
    if scale is not None:
        lo, hi = lo * scale, hi * scale
        lo, hi = torch.minimum(lo, hi), torch.maximum(lo, hi)
        lo, hi = lo - lo.abs() * 2.0 ** -24, hi + hi.abs() * 2.0 ** -24
    lo, hi = round_to(lo, out.dt), round_to(hi, out.dt)
    share = (lo != hi).double().mean().item()
    WIDENED[name] = share
    outside = ((got < lo) | (got > hi)).sum().item()
    fz = gelu64(z) if act == ACT_GELU else (z.clamp(min=0) if act == ACT_RELU else z)
    mid = round_to(fz * (scale if scale is not None else 1.0), out.dt)
    off = ((got != mid) & (lo != hi)).double().mean().item()      # outputs on the end of a two-ended interval that is not round_T(f(z)) itself
    print(f"gemm-ratio {name}: {outside} of {got.numel()} outside their {out.dt} interval, two-ended intervals {100 * share:.3f} %, "
          f"outputs on an end other than round(f(z)) {100 * off:.3f} %")
    if outside:
        i = ((got < lo) | (got > hi)).nonzero()[0].item()
        raise AssertionError(f"{name}: {outside} of {got.numel()} values outside [round(f(z - b)), round(f(z + b))], "
                             f"first: got {got[i].item()!r} for [{lo[i].item()!r}, {hi[i].item()!r}], z = {z[i].item()!r}")


# ---- cases ------------------------------------------------------------------------------------------------------------------------------------------
def case(name, fam, M, N, K, ab, out, exp, form=0, bias=True, res=False, act=ACT_NONE, tag=0, tile=0, max_grid=0, nsplit=0, steps=0,
         coff_bytes=0, **ints):
    """exp = (epilogue, tile, most work items of a workgroup): what the launcher must choose for the case, at 256 and at 64 CUs."""
    return dict(name=name, fam=fam, form=form, M=M, N=N, K=K, ab=ab, out=out, exp=exp, bias=bias, res=res, act=act, tag=tag, tile=tile,
                max_grid=max_grid, nsplit=nsplit, steps=steps, coff_bytes=coff_bytes, **ints)


def _schedule_cases():
    """a. fp32 output through EPI_LIN32 (bias, N % 128 == 0) and EPI_GENERIC (no bias), one XCD slice per workgroup (max_grid = 8): a
    workgroup walks `t` tiles of nk K-steps each, the last row-tile partly empty (M % 16 = 7)."""
    cs = []
    for tile, bm, N in ((1, 64, 128), (2, 128, 512)):
        per_row = N // bm                                         # tiles_n; tiles_m = 8 t / tiles_n
        for nk in (1, 2, 3, 4, 5):
            for t in (1, 2, 3, 4, 6):
                M = bm * (8 * t // per_row) - 9
                for ab in ("bf16", "f16"):
                    for epi, bias in (("LIN32", True), ("GENERIC", False)):
                        cs.append(case(f"sched.t{tile}.nk{nk}.x{t}.{ab}.{epi}", "schedule", M, N, 64 * nk, ab, "f32", (EPI[epi], tile, t), bias=bias,
                                       tile=tile, max_grid=8))
    for ab in ("bf16", "f16"):
        # 8 t + 3 tiles: three XCDs walk one more item than the others
        cs.append(case(f"sched.t1.27tiles.{ab}", "schedule", 64 * 9 - 9, 192, 192, ab, "f32", (EPI["GENERIC"], 1, 4), tile=1, max_grid=8))
        cs.append(case(f"sched.t1.11tiles.{ab}", "schedule", 64 * 11 - 9, 64, 64, ab, "f32", (EPI["GENERIC"], 1, 2), tile=1, max_grid=8))
        cs.append(case(f"sched.t2.27tiles.{ab}", "schedule", 128 * 9 - 9, 384, 128, ab, "f32", (EPI["LIN32"], 2, 4), tile=2, max_grid=8))
        # fewer than 8 tiles: workgroups that own nothing return at once
        cs.append(case(f"sched.t1.4tiles.{ab}", "schedule", 100, 128, 128, ab, "f32", (EPI["LIN32"], 1, 1), tile=1, max_grid=8))
        cs.append(case(f"sched.t2.3tiles.{ab}", "schedule", 300, 128, 64, ab, "f32", (EPI["LIN32"], 2, 1), tile=2))
        # tiles_m = 11, tiles_n = 3: the last rasterisation group has 3 row-blocks
        cs.append(case(f"sched.t1.11x3.{ab}", "schedule", 64 * 11 - 9, 192, 128, ab, "f32", (EPI["GENERIC"], 1, 5), tile=1, max_grid=8))
        cs.append(case(f"sched.t2.11x3.{ab}", "schedule", 128 * 11 - 9, 384, 64, ab, "f32", (EPI["LIN32"], 2, 5), tile=2, max_grid=8))
        # the natural grid with 256 x 256 tiles
        cs.append(case(f"sched.t6.natural.{ab}", "schedule", 300, 256, 64, ab, "f32", (EPI["LIN32"], 6, 1), tile=6))
    return cs


SPLITS = ((5, 3, 2), (4, 4, 1), (5, 2, 3))                       # (nk, nsplit, split_steps)
TILE_EDGE = {1: 64, 2: 128, 6: 256}


def _splitk_cases():
    """b. EPI_PART32 over 8 workgroups (max_grid = 8: workgroup x walks the contiguous slice of XCD x).  The output-tile counts are odd
    (7 x 1 tiles for 3 and 4 ranges, 3 x 3 for 2 ranges), so the boundaries between K-ranges fall INSIDE slices: a workgroup finishes a
    range and goes on in the next one, with another k_beg and, into the short last range, another k_end (splitk_slices;
    tests/test_gemm_family_host.py asserts it for every case).  Every workgroup walks at least two work items."""
    cs = []
    for tile in (2, 6):
        e = TILE_EDGE[tile]
        for nk, ns, st in SPLITS:
            tm, tn = (7, 1) if ns > 2 else (3, 3)
            for ab in ("bf16", "f16"):
                cs.append(case(f"splitk.t{tile}.nk{nk}.{ns}x{st}.{ab}", "splitk", e * tm - 9, e * tn, 64 * nk, ab, "f32",
                               (EPI["PART32"], tile, -(-tm * tn * ns // 8)), bias=False, tile=tile, max_grid=8, nsplit=ns, steps=st))
    return cs


def tile_coords(t, tiles_m, tiles_n, group_m=8):
    """gemm.hip tile_coords: linear tile id -> (row-block, column-block) in grouped order."""
    per_group = group_m * tiles_n
    gid = t // per_group
    first_m = gid * group_m
    gsz = min(tiles_m - first_m, group_m)
    r = t - gid * per_group
    return first_m + r % gsz, r // gsz


def splitk_slices(c):
    """The kernel's persistent schedule for a split-K case (gemm.hip, "persistent, XCD-aware tile schedule"): per workgroup the list of
    its work items as (K-range, row-block, column-block), in the order it walks them."""
    e = TILE_EDGE[c["exp"][1]]
    tiles_m, tiles_n = -(-c["M"] // e), -(-c["N"] // e)
    per_split = tiles_m * tiles_n
    total = per_split * c["nsplit"]
    grid = c["max_grid"]
    assert grid >= 8 and grid % 8 == 0
    wpx, q, r = grid // 8, total // 8, total % 8
    out = []
    for block in range(grid):
        xcd, idx = block % 8, block // 8
        xs = xcd * (q + 1) if xcd < r else r * (q + 1) + (xcd - r) * q
        end = xs + q + (1 if xcd < r else 0)
        out.append([(t // per_split,) + tile_coords(t % per_split, tiles_m, tiles_n) for t in range(xs + idx, end, wpx)])
    return out


def _epilogue_cases():
    """c. every specialised epilogue x tile x operand type at M = 37 (below one tile) and 203 (ragged over several), and the generic
    epilogue on the same kind of data where only N % 128 or the alignment of C differs."""
    cs = []
    for ab in ("bf16", "f16"):
        kinds = [("LIN16", ab, ACT_NONE, 0, False), ("GELU", ab, ACT_GELU, 0, False), ("GELU", ab, ACT_GELU, 1, False),
                 ("LIN32", "f32", ACT_NONE, 0, False), ("RES32", "f32", ACT_NONE, 0, True)]
        if ab == "bf16":
            kinds.append(("F16", "f16", ACT_NONE, 0, False))
        for epi, out, act, tag, res in kinds:
            label = f"{epi}{'.tag1' if tag else ''}"
            for M in (37, 203):
                for tile in (1, 2, 6):
                    cs.append(case(f"epi.{label}.t{tile}.M{M}.{ab}", "epilogue", M, 256, 192, ab, out, (EPI[epi], tile, 1), act=act, tag=tag, res=res,
                                   tile=tile))
                # 256 x 256 asked for at N = 384: the documented fall-back to 128 x 128
                cs.append(case(f"epi.{label}.t6->2.M{M}.{ab}", "epilogue", M, 384, 192, ab, out, (EPI[epi], 2, 1), act=act, tag=tag, res=res, tile=6))
            if tag:
                continue
            for tile in (1, 2):
                cs.append(case(f"epi.generic-of-{label}.N200.t{tile}.{ab}", "epilogue", 203, 200, 192, ab, out, (EPI["GENERIC"], tile, 1), act=act,
                               res=res, tile=tile, cols_of=256))
                cs.append(case(f"epi.generic-of-{label}.C+8B.t{tile}.{ab}", "epilogue", 203, 256, 192, ab, out, (EPI["GENERIC"], tile, 1), act=act,
                               res=res, tile=tile, coff_bytes=8))
        for tile in (1, 2, 6):
            for qs in (0.0, QSCALE):
                # qkv_args takes the model width from the weight: K = heads * 64 = 256
                cs.append(case(f"epi.QKV16.t{tile}.{'scaled' if qs else 'plain'}.{ab}", "qkv", 3 * 37, 768, 256, ab, ab, (EPI["QKV16"], tile, 1), form=1,
                               tile=tile, ntok=37, npad=128, heads=4, qscale=qs))
    return cs


def _gelu_domain_cases():
    return [case(f"gelu-domain.{ab}", "gelu-domain", None, 128, 64, ab, ab, (EPI["GELU"], 1, 1), act=ACT_GELU, tile=1) for ab in ("bf16", "f16")]


def _pixshuf_cases():
    cs = []
    for ab in ("bf16", "f16"):
        for s, ch in ((2, 64), (4, 32), (2, 128)):
            for tile in (1, 2, 6):
                cs.append(case(f"pixshuf.s{s}.ch{ch}.t{tile}.{ab}", "pixshuf", 30, s * s * ch, 128, ab, ab, (EPI["PIX16"], tile, 1), form=2, tile=tile,
                               ho=3, wo=5, s=s, ch=ch))
        cs.append(case(f"pixshuf.s2.ch24.generic.{ab}", "pixshuf", 30, 96, 128, ab, ab, (EPI["GENERIC"], 1, 1), form=2, tile=1, ho=3, wo=5, s=2, ch=24))
    return cs


def _periodic_cases():
    """f. MAP_PERIODIC + RES_PERIODIC have no specialised epilogue: both shapes run the generic one (select_epi), at 128 and at 192 columns."""
    cs = []
    for ab in ("bf16", "f16"):
        for tile in (1, 2):
            cs.append(case(f"periodic.3x9.D128.t{tile}.{ab}", "periodic", 27, 128, 192, ab, "f32", (EPI["GENERIC"], tile, 1), form=3, res=True, tile=tile,
                           p_div=9, p_mul=10, p_off=1, ldr=128))
            cs.append(case(f"periodic.2x36.D192.t{tile}.{ab}", "periodic", 72, 192, 64, ab, "f32", (EPI["GENERIC"], tile, 1), form=3, res=True, tile=tile,
                           p_div=36, p_mul=37, p_off=1, ldr=192))
    return cs


SCHEDULE, SPLITK, EPILOGUE = _schedule_cases(), _splitk_cases(), _epilogue_cases()
GELU_DOMAIN, PIXSHUF, PERIODIC = _gelu_domain_cases(), _pixshuf_cases(), _periodic_cases()
ALL = SCHEDULE + SPLITK + EPILOGUE + GELU_DOMAIN + PIXSHUF + PERIODIC
assert len({c["name"] for c in ALL}) == len(ALL)


def ids(cs):
    return [c["name"] for c in cs]


# ---- inputs (seeded; shared between cases of one shape) --------------------------------------------------------------------------------
_DATA = {}


def _rand(shape, seed, scale=1.0):
    return torch.randn(shape, generator=torch.Generator().manual_seed(seed)) * scale


def gelu_domain_values(ab):
    """Every value of the operand type in [-12, 12] (both zeros among them), the largest finite value and its negative."""
    bits = torch.arange(0, 0x8000, dtype=torch.int32).to(torch.int16).view(TD[ab])
    pos = bits[torch.isfinite(bits.float()) & (bits.float() <= 12.0)]
    big = torch.tensor([torch.finfo(TD[ab]).max], dtype=TD[ab])
    v = torch.cat([pos, -pos, big, -big])
    pad = (-v.numel()) % 64
    return torch.cat([v, torch.zeros(pad, dtype=TD[ab])]).view(-1, 64)


def data(c):
    """A [M, K], W [N, K] in the operand type, bias fp32, residual / table fp32 -- from seeds, cached per shape so that a reference is shared."""
    key = (c["fam"], c["form"], c["M"], c["N"], c["K"], c["ab"], tuple(sorted((k, c[k]) for k in ("s", "ch", "p_div") if k in c)))
    if key in _DATA:
        return _DATA[key]
    dt, N, K = TD[c["ab"]], c["N"], c["K"]
    if c.get("cols_of"):                                          # the generic twin at N % 128 != 0: the first N columns of the specialised case's data
        b = data(dict(c, N=c["cols_of"], cols_of=None))
        d = dict(A=b["A"], W=b["W"][:N].contiguous(), bias=b["bias"][:N].contiguous(), res=b["res"][:, :N].contiguous())
        _DATA[key] = d
        return d
    d = {}
    if c["fam"] == "gelu-domain":
        d["A"] = gelu_domain_values(c["ab"])
        W = torch.zeros(N, K)
        W[torch.arange(64), torch.arange(64)] = 1.0
        d["W"], d["bias"] = W.to(dt), torch.zeros(N)
    else:
        seed = 1000 + 7 * c["M"] + 3 * N + K
        d["A"] = _rand((c["M"], K), seed).to(dt)
        if c["form"] == 2:                                        # the ConvTranspose2d weight [Cin, ch, s, s]; the GEMM operand is its permute
            s, ch = c["s"], c["ch"]
            d["w4"] = _rand((K, ch, s, s), seed + 1, K ** -0.5).to(dt)
            d["W"] = d["w4"].permute(2, 3, 1, 0).reshape(s * s * ch, K).contiguous()
            d["bias"] = _rand((ch,), seed + 2)
        else:
            d["W"] = _rand((N, K), seed + 1, K ** -0.5).to(dt)
            d["bias"] = _rand((N,), seed + 2)
        if c["form"] == 3:
            d["res"] = _rand((c["p_mul"], c["ldr"]), seed + 3)    # pos embedding [ntok, D]
        else:
            d["res"] = _rand((c["M"], N), seed + 3)
    _DATA[key] = d
    return d


def rows(c, d):
    return d["A"].shape[0]


# ---- references ---------------------------------------------------------------------------------------------------------------------------------------
PAD_ROWS = 3


def _lin64(A, W, bias, k0=0, k1=None):
    A64, W64 = A.double()[:, k0:k1], W.double()[:, k0:k1]
    z, S = A64 @ W64.T, A64.abs() @ W64.abs().T
    if bias is not None:
        z, S = z + bias.double(), S + bias.double().abs()
    return z, S


def _embed(shape, must, val):
    t = torch.zeros(shape, dtype=torch.float64)
    t[must] = val.reshape(-1)
    return t


def reference(c, d):
    """-> {buffer name: (shape, must, z fp64, bound fp64)}: z = the value before the activation and the rounding (residual included for
    fp32 outputs), bound = (K_range + 3) 2^-23 S; both payload-shaped, meaningful where `must`."""
    M, N, K = rows(c, d), c["N"], c["K"]
    bias = d["bias"] if c["bias"] else None
    form = c["form"]
    if form == 0 and c["nsplit"] > 1:
        ns, st = c["nsplit"], c["steps"]
        shape = (ns + 1, M + PAD_ROWS, N)                         # one slab more than the launch owns
        must = torch.zeros(shape, dtype=torch.bool)
        must[:ns, :M] = True
        z, b = torch.zeros(shape, dtype=torch.float64), torch.zeros(shape, dtype=torch.float64)
        for s in range(ns):
            k0, k1 = 64 * s * st, min(64 * (s + 1) * st, K)
            zs, Ss = _lin64(d["A"], d["W"], None, k0, k1)
            z[s, :M], b[s, :M] = zs, (k1 - k0 + 3) * U23 * Ss
        return {"C": (shape, must, z, b)}
    if form == 0:
        z, S = _lin64(d["A"], d["W"], bias)
        if c["res"]:
            assert c["act"] == ACT_NONE and c["out"] == "f32"
            z, S = z + d["res"].double(), S + d["res"].double().abs()
        shape = (M + PAD_ROWS, N)
        must = torch.zeros(shape, dtype=torch.bool)
        must[:M] = True
        return {"C": (shape, must, _embed(shape, must, z), _embed(shape, must, (K + 3) * U23 * S))}
    if form == 1:
        z, S = _lin64(d["A"], d["W"], bias)
        H, ntok, npad = c["heads"], c["ntok"], c["npad"]
        B = M // ntok
        out = {}
        perm = lambda t: t.reshape(B, ntok, 3, H, 64).permute(2, 0, 3, 1, 4)      # timm Attention.forward: qkv.reshape(...).permute(2, 0, 3, 1, 4)
        zq, Sq = perm(z), perm(S)
        for i, name in enumerate(("C", "Ck")):
            shape = (B, H, npad, 64)
            must = torch.zeros(shape, dtype=torch.bool)
            must[:, :, :ntok] = True
            out[name] = (shape, must, _embed(shape, must, zq[i]), _embed(shape, must, (K + 3) * U23 * Sq[i]))
        shape = (B, H, 64, npad)                                   # v transposed: the attention's P V operand
        must = torch.zeros(shape, dtype=torch.bool)
        must[..., :ntok] = True
        out["Cv"] = (shape, must, _embed(shape, must, zq[2].transpose(-1, -2)), _embed(shape, must, (K + 3) * U23 * Sq[2].transpose(-1, -2)))
        return out
    if form == 2:
        s, ch, ho, wo = c["s"], c["ch"], c["ho"], c["wo"]
        B = M // (ho * wo)
        x = d["A"].double().reshape(B, ho, wo, K).permute(0, 3, 1, 2)
        z = F.conv_transpose2d(x, d["w4"].double(), d["bias"].double(), stride=s).permute(0, 2, 3, 1)
        S = F.conv_transpose2d(x.abs(), d["w4"].double().abs(), d["bias"].double().abs(), stride=s).permute(0, 2, 3, 1)
        shape = (B, ho * s + 2, wo * s + 2, ch)
        must = torch.zeros(shape, dtype=torch.bool)
        must[:, 1:-1, 1:-1] = True
        return {"C": (shape, must, _embed(shape, must, z), _embed(shape, must, (K + 3) * U23 * S))}
    np_, ntok = c["p_div"], c["p_mul"]
    B = M // np_
    zp, Sp = _lin64(d["A"], d["W"], bias)
    pos = d["res"].double()[:, :N]
    cls = torch.zeros(1, 1, N, dtype=torch.float64)                # the cls rows are another kernel's: any value, they are not compared
    z = torch.cat([cls.expand(B, 1, N), zp.reshape(B, np_, N)], 1) + pos[None]
    S = torch.cat([cls.expand(B, 1, N), Sp.reshape(B, np_, N)], 1) + pos.abs()[None]
    shape = (B, ntok, N)
    must = torch.zeros(shape, dtype=torch.bool)
    must[:, 1:] = True
    return {"C": (shape, must, z, (K + 3) * U23 * S)}


_REF = {}


def reference_cached(c, d):
    key = (id(d), c["form"], c["bias"], c["res"], c["nsplit"], c["steps"], tuple(sorted((k, c[k]) for k in ("ntok", "npad", "heads", "p_mul") if k in c)))
    if key not in _REF:
        _REF[key] = reference(c, d)
    return _REF[key]


def make_outs(c, d, device, fill=None):
    """The guarded buffers of a case.  In place (RES32): the written cells hold the residual."""
    ref = reference_cached(c, d)
    outs = {}
    for name, (shape, must, _, _) in ref.items():
        f = fill
        if c["form"] == 0 and c["res"]:
            f = torch.zeros(shape)
            f[:rows(c, d)] = d["res"]
        esz = 4 if c["out"] == "f32" else 2
        outs[name] = Out(shape, c["out"], must, device, coff=c["coff_bytes"] // esz, fill=f)
    return outs


def check_case(c, d, outs, who=""):
    """Every buffer of the case against its reference: guards, then values."""
    ref = reference_cached(c, d)
    for name, (shape, must, z, b) in ref.items():
        label = f"{who}{c['name']}" + ("" if name == "C" else f".{name}")
        if c["out"] == "f32":
            check_f32(outs[name], z, b, label)
        else:
            scale = c.get("qscale") if name == "C" and c["form"] == 1 and c.get("qscale") else None
            check_16(outs[name], z, b, c["act"], label, scale=scale)
    if c["form"] == 0 and c["nsplit"] > 1:                         # the fp64 sum of the slabs against the whole product
        ns, M = c["nsplit"], rows(c, d)
        shape, must, z, b = ref["C"]
        got = outs["C"].payload().detach().cpu().double()[:ns, :M].sum(0)
        full, _ = _lin64(d["A"], d["W"], None)
        assert_within(got, full, b[:ns, :M].sum(0), f"{who}{c['name']}.sum-of-slabs")


# ---- the C struct ---------------------------------------------------------------------------------------------------------------------------------------
FAKE = 0x7F0000000000         # plan only: pointers are looked at for their alignment, never followed


def struct_of(c, d, ptrs=None):
    """lseg_gemm_case of a case; ptrs: {A, W, bias, res, C, Ck, Cv} device addresses (None: 16-byte aligned fakes for the plan)."""
    p = ptrs or {k: FAKE + 0x100000 * i for i, k in enumerate(("A", "W", "bias", "res", "C", "Ck", "Cv"))}
    if ptrs is None:
        p["C"] += c["coff_bytes"]
    M = rows(c, d) if d is not None else c["M"]
    g = _lib.LSegGemmCase()
    g.form, g.A, g.W, g.C = c["form"], p["A"], p["W"], p["C"]
    g.bias = p["bias"] if c["bias"] else None
    if c["res"]:
        g.residual = p["C"] if c["form"] == 0 else p["res"]        # form 0: in place, like lseg_op_gemm_res32
    if c["form"] == 1:
        g.Ck, g.Cv = p["Ck"], p["Cv"]
    g.M, g.N, g.K, g.ab_dtype, g.out_dtype, g.res_dtype, g.act = M, c["N"], c["K"], LD[c["ab"]], LD[c["out"]], _lib.LSEG_F32, c["act"]
    g.tag, g.tile, g.max_grid = c["tag"], c["tile"], c["max_grid"]
    g.nsplit, g.split_steps = c["nsplit"], c["steps"]
    if c["nsplit"] > 1:
        g.c_split_stride = (M + PAD_ROWS) * c["N"]
    for k in ("ntok", "npad", "heads", "qscale", "ho", "wo", "s", "ch", "p_div", "p_mul", "p_off", "ldr"):
        if k in c:
            setattr(g, k, c[k])
    return g


def plan(lib, g, cus):
    out4 = (C.c_int * 4)()
    r = lib.lseg_op_gemm_ex_plan(C.byref(g), cus, C.byref(out4))
    return r, tuple(out4)


def assert_plan(lib, c, g, cus):
    r, p = plan(lib, g, cus)
    assert r == 0, f"{c['name']}: the plan was refused ({r})"
    assert (p[0], p[1], p[3]) == tuple(c["exp"]), f"{c['name']} at {cus} CUs: runs (epilogue, tile, items) = {(p[0], p[1], p[3])}, written for {c['exp']}"
    return p


# ---- fp32 emulation of the kernel (host self-check), with the wrong variants ---------------------------------------------------------------
def _tile_rows(c):
    return {1: 64, 2: 128, 6: 256}[c["exp"][1]]


def emulate(c, d, wrong=None):
    """Plain fp32 torch with the kernel's own index arithmetic, into guarded CPU buffers.  wrong: one of the variants of
    tests/test_gemm_family_host.py."""
    M, N, K = rows(c, d), c["N"], c["K"]
    dt = TD[c["out"]]
    A, W = d["A"].float(), d["W"].float()
    bias = d["bias"].clone() if c["bias"] else None
    if wrong == "bias+4":
        bias = bias.roll(4)
    if wrong == "next-tile-k0":                                     # the first K-step of a row from the row-tile below
        bm = _tile_rows(c)
        assert M > bm
        A = A.clone()
        A[:M - bm, :64] = d["A"].float()[bm:, :64]
    outs = make_outs(c, d, "cpu")

    def contract(k0, k1):
        if wrong == "drop-last-k":
            k1 = k1 - 64
        return A[:, k0:k1] @ W[:, k0:k1].T if k1 > k0 else torch.zeros(M, N)

    if c["form"] == 0 and c["nsplit"] > 1:
        ns, st = c["nsplit"], c["steps"]
        pay = outs["C"].payload()
        for s in range(ns):
            k0, k1 = 64 * s * st, min(64 * (s + 1) * st, K)
            v = contract(k0, k1)
            if wrong == "short-range-twice" and s == ns - 1:
                v = v + v
            r = torch.arange(M)
            if wrong == "last-row-down":
                r[-1] += 1
            pay[s, r] = v
        if wrong == "stale-range":              # a workgroup that keeps its first item's k_beg / k_end when it walks on into the next K-range
            e = TILE_EDGE[c["exp"][1]]
            for items in splitk_slices(c):
                s0 = items[0][0]
                k0, k1 = 64 * s0 * st, min(64 * (s0 + 1) * st, K)
                for s, mb, nb in items[1:]:
                    if s != s0:
                        rr, cc = slice(mb * e, min((mb + 1) * e, M)), slice(nb * e, min((nb + 1) * e, N))
                        pay[s, rr, cc] = A[rr, k0:k1] @ W[cc, k0:k1].T
        return outs
    v = contract(0, K)
    if bias is not None:
        v = v + (bias.repeat(N // bias.numel()) if c["form"] == 2 else bias)
    if c["act"] == ACT_GELU:
        v = v.clamp(min=0) if wrong == "relu-for-gelu" else gelu64(v.double()).float()
    elif c["act"] == ACT_RELU:
        v = v.clamp(min=0)
    m = torch.arange(M)[:, None]
    n = torch.arange(N)[None, :]
    if c["form"] == 0:
        if c["res"]:
            v = v + d["res"]
        pay = outs["C"].payload()
        r = torch.arange(M)
        if wrong == "last-row-down":
            r[-1] += 1
        pay[r] = v.to(dt)
    elif c["form"] == 1:
        H, ntok, npad, dim = c["heads"], c["ntok"], c["npad"], c["K"]
        b, t = m // ntok, m % ntok
        if wrong == "last-row-down":
            t = t.clone()
            t[-1] += 1
        which, head, e = n // dim, (n % dim) // 64, n % 64
        q = v
        if c.get("qscale"):
            qs = torch.tensor(c["qscale"], dtype=torch.float32)
            q = (v.to(dt).float() * qs) if wrong == "scale-after-rounding" else v * qs
        for i, name in enumerate(("C", "Ck")):
            sel = (which == i).expand(M, N)
            src = (q if i == 0 else v).to(dt)
            outs[name].payload()[b.expand(M, N)[sel], head.expand(M, N)[sel], t.expand(M, N)[sel], e.expand(M, N)[sel]] = src[sel]
        sel = (which == 2).expand(M, N)
        outs["Cv"].payload()[b.expand(M, N)[sel], head.expand(M, N)[sel], e.expand(M, N)[sel], t.expand(M, N)[sel]] = v.to(dt)[sel]
    elif c["form"] == 2:
        s, ch, ho, wo = c["s"], c["ch"], c["ho"], c["wo"]
        b, y, x = m // (ho * wo), (m % (ho * wo)) // wo, m % wo
        down = torch.zeros_like(m)
        if wrong == "last-row-down":
            down[-1] = 1
        i, j, co = (n // ch) // s, (n // ch) % s, n % ch
        if wrong == "ij-transposed":
            i, j = j, i
        e = lambda t: t.expand(M, N).reshape(-1)
        outs["C"].payload()[e(b), e(y * s + i + 1 + down), e(x * s + j + 1), e(co)] = v.to(dt).reshape(-1)
    else:
        p_div, p_mul, p_off = c["p_div"], c["p_mul"], (0 if wrong == "p_off=0" else c["p_off"])
        r = torch.arange(M)
        row = (r // p_div) * p_mul + r % p_div + p_off
        if wrong == "last-row-down":
            row[p_div - 1] += 1                                     # the first image's last patch: onto the next image's cls row
        v = v + d["res"][r % p_div + p_off, :N]
        outs["C"].payload().view(-1, N)[row] = v.to(dt)
    return outs
