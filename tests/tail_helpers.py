"""References, bounds and comparisons for the output tail: the 2x2-cell gram, the per-pixel norm plane, the scaled x2 / one-pass x4
upsample of the label planes, output_conv's x2 and the strict tail's upsample + normalise (csrc/elementwise.hip, csrc/corr.hip).

Same method as tests/glue_helpers.py, whose comparisons this file reuses: every reference is plain fp64 torch on the CPU from the same
16-bit / fp32 inputs, every fp32 result is held to `gamma(k) * sum|terms|` with the sum taken from the fp64 reference and k counted
from the kernel's longest path (gamma(k) = k u / (1 - k u), u = 2^-24: k roundings to nearest compound to at most that), and every
fp16 rounding is held to an INTERVAL: the value must be fp16-representable and lie in [fp16(ref - b), fp16(ref + b)], b the counted
fp32 bound of the value before the rounding (rounding to nearest is monotone, so a correct kernel cannot leave it).  The two ends are
built with numpy from float64 (one rounding; torch's .half() of a double rounds twice, through fp32).  An interval is "widened" where its
ends differ; the share of widened intervals is a property of the inputs alone and is capped at 1 % (WIDENED_CAP), so that at least 99 %
of the elements are held to one exact bit pattern.  tests/test_output_tail_host.py checks that cap on the CPU for every case the GPU
file runs, and shows that fp32 emulations of the kernels pass these comparisons while wrong variants fail them.

Bilinear coordinate.  The kernels form the align_corners=True source coordinate in fp32: r = fl((n-1) / (2n-1)), s = fl(r * i), each
one rounding at the magnitude of s, so |s - src| <= 2 u (1 + u) src ABSOLUTE, and the fraction l = s - floor(s) (exact) inherits that:
it is not one rounding of the fraction.  The output is linear in each fraction, so the bound carries
dsrc_y * sum_x wx |v[y1, x] - v[y0, x]| + dsrc_x * sum_y wy |v[y, x1] - v[y, x0]| (ac_taps / up2_ref), as pos_resize_ref does.
No tap can change under that error: src = i (n-1) / (2n-1) is an integer only at i = 0 and i = 2n-1 (gcd(n-1, 2n-1) = 1) and is
otherwise at least 1 / (2n-1) away from one.  At i = 2n-1 the fp32 product lands exactly on n-1 (checked for every n in 2..1100 by
test_output_tail_host.py), both taps are the last cell and the difference in the coordinate term is 0.
"""
import numpy as np
import torch
import torch.nn.functional as F

from glue_helpers import U24, RATIOS, Guarded, assert_bits_equal, assert_within, randn  # noqa: F401  (re-exported to the tests)

WIDENED_CAP = 0.01
WIDENED = {}             # case name -> share of widened fp16 intervals (printed per case)
RSQRT_ULPS = 1           # HIP math API, single precision device functions: rsqrtf, sqrtf and the division are listed at <= 1 ulp
F32 = torch.float32


def gamma(k):
    return k * U24 / (1 - k * U24)


# ---- align_corners=True x2 taps ---------------------------------------------------------------------------------------------------------
def ac_taps(n, align_corners=True):
    """One axis of the x2 bilinear n -> 2n in fp64: (i0, i1, l, Wt [2n, n] tap weights, Dt [2n, n] = d Wt / d src, dsrc [2n])."""
    no = 2 * n
    i = torch.arange(no, dtype=torch.float64)
    src = i * (n - 1) / (no - 1) if align_corners else ((i + 0.5) / 2 - 0.5).clamp(min=0)
    i0 = src.floor().long().clamp(max=n - 1)
    i1 = (i0 + 1).clamp(max=n - 1)
    l = src - i0
    r = torch.arange(no)
    Wt = torch.zeros(no, n, dtype=torch.float64)
    Wt[r, i0] += 1 - l
    Wt[r, i1] += l
    Dt = torch.zeros(no, n, dtype=torch.float64)
    Dt[r, i0] -= 1
    Dt[r, i1] += 1
    return i0, i1, l, Wt, Dt, 2 * U24 * (1 + U24) * src


def up2_ref(v, align_corners=True):
    """v [..., H, W] -> (ref [..., 2H, 2W] fp64, mag = the same resize of |v| (the weights are >= 0), coord = the coordinate term)."""
    v = v.double()
    H, W = v.shape[-2:]
    _, _, _, Wy, Dy, ey = ac_taps(H, align_corners)
    _, _, _, Wx, Dx, ex = ac_taps(W, align_corners)
    ref = torch.einsum("ya,...ab,xb->...yx", Wy, v, Wx)
    mag = torch.einsum("ya,...ab,xb->...yx", Wy, v.abs(), Wx)
    sy = torch.einsum("xb,...yb->...yx", Wx, torch.einsum("ya,...ab->...yb", Dy, v).abs()) * ey[:, None]
    sx = torch.einsum("ya,...ax->...yx", Wy, torch.einsum("xb,...ab->...ax", Dx, v).abs()) * ex[None, :]
    return ref, mag, sy + sx


def up2_planes_ref(v):
    """upsample2x_planes_kernel / the second half of the one-pass x4: bilerp() = fma(ly, h1, wy h0), h = fma(lx, b, wx a).  Longest path
    of a tap: wx = 1 - lx, wx a, the fma, wy = 1 - ly, wy h0, the fma: 6 roundings.  -> (ref, bound)."""
    ref, mag, coord = up2_ref(v)
    return ref, gamma(6) * mag + coord


# ---- fp16 intervals -------------------------------------------------------------------------------------------------------------------------
def f16_ends(ref64, b64):
    lo = torch.from_numpy((ref64 - b64).numpy().astype(np.float16))
    hi = torch.from_numpy((ref64 + b64).numpy().astype(np.float16))
    return lo, hi


def widened_share(lo, hi):
    return (lo != hi).double().mean().item()


def assert_f16_interval(got, lo, hi, name):
    """`got`: fp16, or fp32 holding fp16 values.  Representable, inside [lo, hi]; the widened share is printed and capped."""
    g = got.detach().cpu()
    assert tuple(g.shape) == tuple(lo.shape), f"{name}: shape {tuple(g.shape)} vs {tuple(lo.shape)}"
    assert torch.isfinite(g.float()).all(), f"{name}: non-finite output (an element was not written?)"
    if g.dtype != torch.float16:
        assert torch.equal(g.half().to(g.dtype), g), f"{name}: a value is not fp16-representable (the rounding is missing)"
    g64 = g.double()
    share = widened_share(lo, hi)
    WIDENED[name] = share
    outside = ((g64 < lo.double()) | (g64 > hi.double())).sum().item()
    print(f"glue-ratio {name}: {outside} of {g.numel()} outside their fp16 interval, widened intervals {100 * share:.3f} %")
    assert share <= WIDENED_CAP, f"{name}: {100 * share:.3f} % of the fp16 intervals are widened: the inputs break the 1 % cap"
    assert outside == 0, f"{name}: {outside} of {g.numel()} values outside [fp16(ref - b), fp16(ref + b)]"


# ---- a. the 2x2-cell gram ---------------------------------------------------------------------------------------------------------------------
def gram_ref(g16pad, swap_diag_anti=False):
    """g fp16 padded NHWC [B, H+2, W+2, C] -> (gram [B, H, W, 5] fp64 = {q.q, q.right, q.down, q.diag, right.down}, sum|products|).
    The border takes part in the last row's and column's records (the products of test_corr_planes_kernel)."""
    gd = g16pad.double()
    a, r, d, dr = gd[:, 1:-1, 1:-1], gd[:, 1:-1, 2:], gd[:, 2:, 1:-1], gd[:, 2:, 2:]
    pairs = [(a, a), (a, r), (a, d), (a, dr), (r, d)]
    if swap_diag_anti:
        pairs[3], pairs[4] = pairs[4], pairs[3]
    return torch.stack([(p * q).sum(-1) for p, q in pairs], -1), torch.stack([(p * q).abs().sum(-1) for p, q in pairs], -1)


def gram_bound(mag, C):
    """pixel_gram_kernel: a product of two fp16 values is exact in fp32 (22 significant bits), so only the additions round: a lane adds
    its 8 NV products in order (the first lands on 0: <= 8 NV roundings on the first product's path), then 6 shuffle levels:
    k = 8 NV + 6, NV = 1 for C <= 512, 2 above."""
    return gamma(8 * (1 if C <= 512 else 2) + 6) * mag


# ---- b. the norm plane --------------------------------------------------------------------------------------------------------------------------
def _cell_weights(H, W, dt=torch.float64):
    y0, y1, ly, _, _, _ = ac_taps(H)
    x0, x1, lx, _, _, _ = ac_taps(W)
    ly, lx = ly.to(dt)[:, None], lx.to(dt)[None, :]
    return (y0, y1, x0, x1), ((1 - ly) * (1 - lx), (1 - ly) * lx, ly * (1 - lx), ly * lx)


def quad_terms(gram, idx, w, swap_bc_bd=False, cross=2.0):
    """The 10 terms of ||u||^2 = sum_i w_i^2 g_i.g_i + 2 sum_{i<j} w_i w_j g_i.g_j over the cell a = (y0, x0), b = (y0, x1),
    c = (y1, x0), d = (y1, x1), from the gram records [B, H, W, 5] in gram's dtype: a.b = ra[1], a.c = ra[2], a.d = ra[3], b.c = ra[4],
    b.d = rb[2], c.d = rc[1]."""
    y0, y1, x0, x1 = idx
    wa, wb, wc, wd = w
    ra, rb, rc, rd = gram[:, y0][:, :, x0], gram[:, y0][:, :, x1], gram[:, y1][:, :, x0], gram[:, y1][:, :, x1]
    bc, bd = (rb[..., 2], ra[..., 4]) if swap_bc_bd else (ra[..., 4], rb[..., 2])
    diag = [wa * wa * ra[..., 0], wb * wb * rb[..., 0], wc * wc * rc[..., 0], wd * wd * rd[..., 0]]
    crs = [wa * wb * ra[..., 1], wa * wc * ra[..., 2], wa * wd * ra[..., 3], wb * wc * bc, wb * wd * bd, wc * wd * rc[..., 1]]
    return diag, [cross * t for t in crs]


def norm_plane_ref(g16pad, s):
    """-> (gram [B, H, W, 5] fp32: the fp64 gram of g rounded once; ref [B, 2H, 2W] fp64 = s / ||bilinear_fp64(g)||; its bound; n2; form,
    the fp64 quadratic form over the unrounded gram, which must equal n2 -- the reference's own check of the pairing).
    n2, absolute: k = 14 on the longest path, a cross term: wa = fl(fl(1-ly) fl(1-lx)) 3 roundings, wb 2, their product 1, times the
    record 1, the record's own rounding to fp32 1, 5 additions inside the cross group, the doubling exact, the last addition 1
    (a squared term: 3 + 3 + 1 + 1 + 1 + 3 + 1 = 13).  b_n2 = gamma(14) sum|terms| + the coordinate term
    2 |u . du/dly| dsrc_y + 2 |u . du/dlx| dsrc_x.  The factor: d(n2^-1/2) / n2^-1/2 = 0.5 b / n2 (times 1 + b / n2 for the curvature),
    rsqrtf within RSQRT_ULPS ulp = 2 RSQRT_ULPS u, the product with s one rounding."""
    gd = g16pad.double()
    H, W = gd.shape[1] - 2, gd.shape[2] - 2
    gram64, _ = gram_ref(g16pad)
    gi = gd[:, 1:-1, 1:-1].permute(0, 3, 1, 2)
    _, _, _, Wy, Dy, ey = ac_taps(H)
    _, _, _, Wx, Dx, ex = ac_taps(W)
    u = torch.einsum("ya,bcax,Xx->bcyX", Wy, gi, Wx)
    uy = torch.einsum("ya,bcax,Xx->bcyX", Dy, gi, Wx)
    ux = torch.einsum("ya,bcax,Xx->bcyX", Wy, gi, Dx)
    n2 = (u * u).sum(1)
    coord = 2 * ((u * uy).sum(1).abs() * ey[:, None] + (u * ux).sum(1).abs() * ex[None, :])
    idx, w = _cell_weights(H, W)
    diag, crs = quad_terms(gram64, idx, w)
    form = sum(diag) + sum(crs)
    mag = sum(t.abs() for t in diag) + sum(t.abs() for t in crs)
    b_n2 = gamma(14) * mag + coord
    ref = s / n2.sqrt()
    bound = ref.abs() * (0.5 * (b_n2 / n2) * (1 + b_n2 / n2) + (2 * RSQRT_ULPS + 1) * U24)
    return gram64.float(), ref, bound, n2, form


def footprint(H, W, y, x):
    """Output pixels [2H, 2W] of the norm plane that address gram record (y, x) through any of their four taps (weight 0 included)."""
    (y0, y1, x0, x1), _ = _cell_weights(H, W)
    return ((y0 == y) | (y1 == y))[:, None] & ((x0 == x) | (x1 == x))[None, :]


# ---- c. the scaled x2 and the one-pass x4 ------------------------------------------------------------------------------------------------------
def smooth_planes(P, H, W, seed, amp):
    """Label planes 5 (m_p + amp (field + noise)), |m_p| in 1..2 with alternating sign: what t_k . g_p looks like on a feature map -- a
    level per label, neighbours `amp` of it apart.  The coordinate term is up to 2 u src |b - a| whatever the value is, and the fp16
    spacing follows the value: planes that cross zero, or whose neighbours differ by their own magnitude at src ~ 100, widen more than
    1 % of the intervals (measured on the reference alone: 8 % at W = 130 for independent N(0, 5) pixels)."""
    gen = torch.Generator().manual_seed(seed)
    mean = (1 + torch.rand((P, 1, 1), generator=gen)) * (1 - 2 * (torch.arange(P) % 2)).view(P, 1, 1)
    coarse = randn((1, P, (H + 3) // 4 + 1, (W + 3) // 4 + 1), seed + 1)
    base = F.interpolate(coarse, size=(H, W), mode="bilinear", align_corners=True)[0]
    return (5 * (mean + amp * (base + randn((P, H, W), seed + 2)))).float()


def pad_nan(v):
    """[P, H, W] -> [P, H+2, W+2] with a NaN border: a kernel that read it could not meet any bound."""
    out = torch.full((v.shape[0], v.shape[1] + 2, v.shape[2] + 2), float("nan"), dtype=v.dtype)
    out[:, 1:-1, 1:-1] = v
    return out


def low_ref(R, scale, K, align_corners=True, image0_scale=False):
    """R [B*K, H, W] fp32, scale [B, 2H, 2W] fp32 -> (lo, hi) fp16 ends of low = fp16(scale[p / K] * bilerp(R[p])) [B*K, 2H, 2W].
    b = |scale| (gamma(7) mag + coord): bilerp's 6 roundings and the product's 1 (pinned to an fp32 register: ups_low_value)."""
    ref, mag, coord = up2_ref(R, align_corners)
    sc = scale.double().repeat_interleave(K, 0)
    if image0_scale:
        sc = scale.double()[:1].expand(R.shape[0], -1, -1)
    return f16_ends(sc * ref, sc.abs() * (gamma(7) * mag + coord))


def check_x4_tail(low, out_two, out_one, R, scale, K, case, who="upsample4x"):
    """The three assertions of the x4 tail on (low_scratch of the two-stage form, its output, the one-pass output):
    1. low inside its fp16 intervals;  2. one pass == two stages, bit for bit;  3. the output within up2_planes_ref of the low it was
    made from (stage 1 was checked in 1., so stage 2 is checked on its own)."""
    lo, hi = low_ref(R, scale, K)
    assert_f16_interval(low, lo, hi, f"{who}.low[{case}]")
    assert_bits_equal(out_one.detach().cpu(), out_two.detach().cpu(), f"{who}.one_pass_vs_two_stage[{case}]")
    ref, bound = up2_planes_ref(low.detach().cpu())
    assert_within(out_two, ref, bound, f"{who}.x2_of_low[{case}]")


# ---- e. upsample + normalise + the two fp16 roundings ----------------------------------------------------------------------------------------
def _scaled_f16(q16, scale):
    """The two roundings a kernel may apply to the exact product scale * q16: straight to fp16, or to fp32 first."""
    m = scale * q16.double()
    direct = torch.from_numpy(m.numpy().astype(np.float16))
    via32 = torch.from_numpy(m.float().numpy().astype(np.float16))
    return direct, via32


def upsample_norm_ref(g32pad, scale):
    """g fp32 padded NHWC [B, H+2, W+2, C] (border unread) -> (lo, hi) fp16 [B, 2H, 2W, C] around fp16(scale * fp16(u / ||u||)).
    u: the bilinear's 6 roundings + the coordinate term (b_u).  s2 = sum u^2: the square 1, a lane's 8 NV additions, 6 shuffle levels:
    gamma(8 NV + 7) s2, plus 2 sum|u| b_u carried from u.  nrm = sqrtf(s2): 0.5 b_s2 / s2 + 1 ulp; the division 1 ulp.  First fp16
    rounding: q in [fp16(q - b_q), fp16(q + b_q)].  Second: scale * q16 is exact in fp64 (24 + 11 bits); the kernel rounds it to fp32 and
    then to fp16, or -- where the compiler fuses product and conversion (v_fma_mixlo_f16, cf. ups_low_value in common.h) -- once to fp16:
    both results are allowed and nothing else (_scaled_f16).  They differ where the exact product is within an fp32 rounding of an fp16
    tie.  For scale = fp32(1 / 0.07) = 100 / 7 (1 - 1e-8) that is 4 % of all fp16 values (every q16 whose significand is an odd multiple
    of 7 gives 12.5 t (1 - 1e-8)), so the production scale would break the 1 % cap by itself: the cases use UPNORM_SCALE, which has no
    small rational nearby."""
    assert scale > 0
    g = g32pad[:, 1:-1, 1:-1].double().permute(0, 3, 1, 2)
    C = g.shape[1]
    u, mag, coord = up2_ref(g)
    b_u = gamma(6) * mag + coord
    s2 = (u * u).sum(1, keepdim=True)
    b_s2 = gamma(8 * (1 if C <= 512 else 2) + 7) * s2 + 2 * (u.abs() * b_u).sum(1, keepdim=True)
    nrm = s2.sqrt()
    rel_n = 0.5 * (b_s2 / s2) * (1 + b_s2 / s2) + 2 * RSQRT_ULPS * U24
    q = u / nrm
    b_q = (b_u / nrm + q.abs() * (rel_n + 2 * RSQRT_ULPS * U24)) * (1 + 1e-6)
    qlo, qhi = f16_ends(q, b_q)
    lo = torch.minimum(*_scaled_f16(qlo, scale))
    hi = torch.maximum(*_scaled_f16(qhi, scale))
    return lo.permute(0, 2, 3, 1).contiguous(), hi.permute(0, 2, 3, 1).contiguous()


def feature_map(B, H, W, C, seed, rough, dtype):
    """A padded NHWC feature map whose interior pixels share a direction up to `rough` (rough = None: independent pixels)."""
    noise = randn((B, H + 2, W + 2, C), seed)
    if rough is None:
        return noise.to(dtype)
    return (randn((B, 1, 1, C), seed + 1) + rough * noise).to(dtype)


# ---- fp32 emulations of the kernels on the host (test_output_tail_host.py) -------------------------------------------------------------------
def taps_f32(n, align_corners=True, fused=False):
    """src_tap() in fp32: r = (n-1) / (2n-1), s = r * i (rounded), i0 = (int)s, i1 = i0 + (i0 < n-1), l = s - i0.
    fused: l = fma(r, i, -i0), what a compiler makes of the same lines without `fp contract(off)`: the last index gets the exact
    product's remainder instead of 0, on a clamped tap."""
    i = torch.arange(2 * n).to(F32)
    r = torch.tensor(float(n - 1), dtype=F32) / torch.tensor(float(2 * n - 1), dtype=F32)
    s = r * i if align_corners else ((i + 0.5) * 0.5 - 0.5).clamp(min=0)
    i0 = s.to(torch.int64)
    l = (r.double() * i.double() - i0.double()).float() if fused else s - i0.to(F32)
    return i0, i0 + (i0 < n - 1).long(), l


def emu_bilerp(v, align_corners=True, ytaps=None):
    """bilerp() of planes [..., H, W] fp32 -> [..., 2H, 2W] fp32 (separate multiply and add: an fma only removes roundings)."""
    H, W = v.shape[-2:]
    y0, y1, ly = ytaps if ytaps is not None else taps_f32(H, align_corners)
    x0, x1, lx = taps_f32(W, align_corners)
    ly = ly[:, None]
    r0, r1 = v[..., y0, :], v[..., y1, :]
    h0 = lx * r0[..., x1] + (1 - lx) * r0[..., x0]
    h1 = lx * r1[..., x1] + (1 - lx) * r1[..., x0]
    return ly * h1 + (1 - ly) * h0


def emu_low(R, scale, K, align_corners=True, round16=True, image0_scale=False):
    sc = scale[:1].expand(R.shape[0], -1, -1) if image0_scale else scale.repeat_interleave(K, 0)
    m = sc * emu_bilerp(R, align_corners)
    return m.half().float() if round16 else m


def emu_norm_plane(gram32, H, W, s, swap_bc_bd=False, cross=2.0, fused=False):
    y0, y1, ly = taps_f32(H, fused=fused)
    x0, x1, lx = taps_f32(W, fused=fused)
    ly, lx = ly[:, None], lx[None, :]
    w = ((1 - ly) * (1 - lx), (1 - ly) * lx, ly * (1 - lx), ly * lx)
    diag, crs = quad_terms(gram32, (y0, y1, x0, x1), w, swap_bc_bd, 1.0)
    n2 = (diag[0] + diag[1] + diag[2] + diag[3]) + torch.tensor(cross, dtype=F32) * (crs[0] + crs[1] + crs[2] + crs[3] + crs[4] + crs[5])
    return torch.tensor(s, dtype=F32) * torch.rsqrt(n2)


def emu_gram(g16pad, swap_diag_anti=False):
    """fp32 sums of the exact products in another order than the kernel's: still inside the counted bound."""
    g = g16pad.float()
    a, r, d, dr = g[:, 1:-1, 1:-1], g[:, 1:-1, 2:], g[:, 2:, 1:-1], g[:, 2:, 2:]
    pairs = [(a, a), (a, r), (a, d), (a, dr), (r, d)]
    if swap_diag_anti:
        pairs[3], pairs[4] = pairs[4], pairs[3]
    return torch.stack([(p * q).reshape(*p.shape[:-1], -1, 8).sum(-1).sum(-1) for p, q in pairs], -1)


def emu_upsample_norm(g32pad, scale, norm_first=False):
    g = g32pad[:, 1:-1, 1:-1].permute(0, 3, 1, 2).contiguous()
    if norm_first:
        g = g / (g * g).sum(1, keepdim=True).sqrt()
    u = emu_bilerp(g)
    q = u if norm_first else u / (u * u).sum(1, keepdim=True).sqrt()
    return (torch.tensor(scale, dtype=F32) * q.half().float()).half().permute(0, 2, 3, 1).contiguous()


# ---- the cases both test files run (the GPU file on the kernels, the host file on the emulations and on the 1 % cap) ----------------------------
GRAM_SHAPES = [(1, 1, 1, 8), (2, 3, 5, 64), (1, 4, 6, 512), (1, 2, 7, 520), (1, 3, 4, 1024), (3, 5, 9, 768)]
NORM_SHAPES = [(1, 2, 2), (2, 3, 7), (1, 8, 5), (2, 17, 30)]
X4_SHAPES = [(1, 1, 2, 2), (2, 3, 7, 6), (1, 2, 8, 16), (1, 2, 9, 30), (1, 1, 17, 34), (1, 1, 12, 130), (1, 1, 3, 258), (2, 5, 33, 10)]
X2_SHAPES = [(1, 2, 4), (3, 5, 8), (7, 24, 20), (2, 9, 132)]
UPNORM_SHAPES = [(1, 2, 2, 8), (2, 3, 5, 64), (1, 4, 3, 512), (1, 2, 3, 768), (1, 2, 2, 1024)]
LOGIT_SCALE = float(np.float32(1 / 0.07))
UPNORM_SCALE = float(np.float32(8 * 2 ** 0.5))


def x4_inputs(B, K, H, W):
    """(R [B*K, H, W] fp32, scale [B, 2H, 2W] fp32 in 8..12).  The roughness falls with the size, as the coordinate term grows with it."""
    R = smooth_planes(B * K, H, W, 300 + H + W, min(0.3, 8.0 / (H + W)))
    scale = 8 + 4 * torch.rand((B, 2 * H, 2 * W), generator=torch.Generator().manual_seed(301 + H + W))
    return R, scale


def upnorm_input(B, H, W, C):
    g = feature_map(B, H, W, C, 400 + C, 0.5, F32)
    g[:, 0], g[:, -1], g[:, :, 0], g[:, :, -1] = float("nan"), float("nan"), float("nan"), float("nan")
    return g
