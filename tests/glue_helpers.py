"""References and comparisons for the training backward's data-movement ("glue") kernels.

Every reference is plain torch in fp64 on the CPU; every comparison is exact (bit patterns) or a bound counted from the kernel's
operations, `k * 2^-24 * sum|terms|` with the sum taken from the fp64 reference, never from the output under test.  The GPU tests
(tests/test_gpu_train_glue.py) and the host self-check (tests/test_train_glue_host.py, which feeds deliberately wrong torch variants
through the same functions) share this file, so a bar that the host test shows to be tight is the bar the kernels are held to.

Unit: one fp32 rounding to nearest moves a value by at most 2^-24 of its magnitude (half an ulp, reached just above a power of two);
the counts next to the bounds are counts of such roundings on the longest path of any one term.
"""
import torch
import torch.nn.functional as F

U24 = 2.0 ** -24
RATIOS = {}              # kernel name -> worst err / bound seen in this process (also printed per case)


# ---- comparisons ------------------------------------------------------------------------------------------------------------------
def _bits(t):
    t = t.detach().cpu().contiguous()
    return t.view({2: torch.int16, 4: torch.int32, 8: torch.int64}[t.element_size()])


def assert_bits_equal(got, ref, name):
    """torch.equal on the bit patterns: -0.0 != +0.0, a subnormal must survive, NaN payloads count."""
    assert got.shape == ref.shape and got.dtype == ref.dtype, f"{name}: {tuple(got.shape)} {got.dtype} vs {tuple(ref.shape)} {ref.dtype}"
    g, r = _bits(got), _bits(ref)
    if not torch.equal(g, r):
        bad = (g != r).nonzero()
        raise AssertionError(f"{name}: {bad.shape[0]} of {g.numel()} elements differ bitwise, first at {bad[0].tolist()}")


def assert_within(got, ref64, bound64, name):
    """|got - ref| <= bound element-wise (a zero bound demands equality); prints and records the worst err / bound."""
    assert tuple(got.shape) == tuple(ref64.shape), f"{name}: shape {tuple(got.shape)} vs {tuple(ref64.shape)}"
    g = got.detach().cpu().double()
    assert torch.isfinite(g).all(), f"{name}: non-finite output (an element was not written?)"
    err = (g - ref64).abs()
    zero = bound64 <= 0
    assert (err[zero] == 0).all(), f"{name}: an element with a zero bound is not exact"
    ratio = (err[~zero] / bound64[~zero]).max().item() if (~zero).any() else 0.0
    RATIOS[name.split("[")[0]] = max(RATIOS.get(name.split("[")[0], 0.0), ratio)
    print(f"glue-ratio {name}: worst err/bound = {ratio:.4f}")
    assert ratio <= 1.0, f"{name}: worst err/bound = {ratio:.4f} > 1"
    return ratio


def assert_max_err(got, ref64, lim, name):
    """max|got - ref| <= lim: the form of the bars in test_linear_backward / test_conv3x3_backward."""
    g = got.detach().cpu().double()
    assert torch.isfinite(g).all(), f"{name}: non-finite output"
    err = (g - ref64).abs().max().item()
    print(f"glue-ratio {name}: max err {err:.3e} / bar {lim:.3e} = {err / lim:.4f}")
    assert err <= lim, f"{name}: {err} > {lim}"


# ---- guarded output buffers ------------------------------------------------------------------------------------------------------------
GUARD = 64               # elements on each side: 128 B (16-bit) / 256 B (fp32), so the payload keeps its 16-byte alignment
SENTINEL16 = 0x7FC1      # a NaN in bf16 and in fp16 that neither rounding produces


class Guarded:
    """A flat device buffer [guard | payload | guard] filled with a NaN sentinel; `t` is the payload view handed to the kernel."""

    def __init__(self, shape, dtype, device="cuda", fill=None):
        n = 1
        for s in shape:
            n *= s
        self.n, self.dtype = n, dtype
        if dtype in (torch.bfloat16, torch.float16):
            self.buf = torch.full((n + 2 * GUARD,), SENTINEL16, dtype=torch.int16, device=device).view(dtype)
        else:
            self.buf = torch.full((n + 2 * GUARD,), float("nan"), dtype=dtype, device=device)
        self.t = self.buf[GUARD:GUARD + n].view(shape)
        if fill is not None:
            self.t.copy_(fill)
        self.before = self.buf.clone()

    def check(self, name, written=True):
        """Nothing outside the payload was touched; with `written`, no payload element still holds the sentinel."""
        b, a = _bits(self.before), _bits(self.buf)
        assert torch.equal(a[:GUARD], b[:GUARD]) and torch.equal(a[-GUARD:], b[-GUARD:]), f"{name}: wrote outside its output"
        if written:
            pay = self.buf[GUARD:GUARD + self.n].cpu()
            assert not torch.isnan(pay.float()).any(), f"{name}: an output element was not written"

    def untouched(self, name):
        assert torch.equal(_bits(self.before), _bits(self.buf)), f"{name}: a refused call wrote to its output"


# ---- inputs -----------------------------------------------------------------------------------------------------------------------------
def randn(shape, seed, scale=1.0, dtype=torch.float32):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(shape, generator=g) * scale).to(dtype)


def with_specials16(t):
    """Plant -0.0, the smallest subnormal and its negative into a 16-bit tensor (a copy kernel must carry the bits)."""
    v = t.contiguous().view(-1).view(torch.int16)
    n = v.numel()
    for k, bits in enumerate((-0x8000, 0x0001, -0x7FFF)):
        v[(k * 7919 + 3) % n] = bits
    return t


# ---- pos-embed resize (lseg_vit.py:149-163) ------------------------------------------------------------------------------------------
def pos_taps_1d(n_in, n_out):
    """One axis of the align_corners=False resize in fp64: (Wt [n_out, n_in] tap weights, Dt [n_out, n_in] = d Wt / d src: -1 at
    the lower tap, +1 at the upper, 0 where both clamp to the last cell, dsrc [n_out]).
    dsrc bounds the error of the fp32 source coordinate s = max(0, (i + 0.5) * (n_in / n_out) - 0.5), which is what PyTorch's fp32
    resize and the kernels compute: the quotient is rounded (2^-24, relative) and the product is rounded (2^-24), both at the magnitude
    src + 0.5, and the subtraction is rounded at the magnitude src <= src + 0.5 (2^-24): |s - src| <= 3 * 2^-24 * (src + 0.5).
    The fraction l = s - floor(s) is then exact and inherits that absolute error: it is NOT one rounding of the fraction (2^-24 * l),
    which is what a count of "one rounding for the source coordinate" would allow.  (A fused multiply-add only removes roundings.)"""
    i = torch.arange(n_out, dtype=torch.float64)
    a = (i + 0.5) * n_in / n_out
    src = (a - 0.5).clamp(min=0)
    i0 = src.floor().long().clamp(max=n_in - 1)
    i1 = (i0 + 1).clamp(max=n_in - 1)
    l = src - i0
    r = torch.arange(n_out)
    Wt = torch.zeros(n_out, n_in, dtype=torch.float64)
    Wt[r, i0] += 1 - l
    Wt[r, i1] += l
    Dt = torch.zeros(n_out, n_in, dtype=torch.float64)
    Dt[r, i0] -= 1
    Dt[r, i1] += 1
    return Wt, Dt, 3 * U24 * a


def pos_resize_ref(pos, g_old, gh, gw, align_corners=False, coord_term=True):
    """pos [1+g_old^2, D] -> (ref [1+gh*gw, D] fp64, bound).  Row 0 is a copy (bound 0); the grid rows are F.interpolate in fp64.
    Bound: 8 * 2^-24 * sum|w v| over the four taps (the weights are >= 0, so that sum is the same resize of |v|) for the fp32
    roundings of the interpolation expression -- 1-lx, product, sum, 1-ly, product, sum: 6 on any tap's path, inside the 7 + 1 the
    bar was first written with -- plus what that first count missed (coord_term=False leaves it out, to show the miss):
    the source coordinate's rounding at its own magnitude (pos_taps_1d), which moves the output by at most
    dsrc_y * sum_x wx |v[y1, x] - v[y0, x]| + dsrc_x * sum_y wy |v[y, x1] - v[y, x0]|, the resize being linear in each fraction and
    continuous across a tap change.  Every sum is over the fp64 reference's taps."""
    D = pos.shape[1]
    p = pos.double()

    def rs(g):
        g = g.reshape(1, g_old, g_old, D).permute(0, 3, 1, 2)
        o = F.interpolate(g, size=(gh, gw), mode="bilinear", align_corners=align_corners)
        return o.permute(0, 2, 3, 1).reshape(gh * gw, D)

    ref = torch.cat([p[:1], rs(p[1:])], 0)
    bound = 8 * U24 * rs(p[1:].abs())
    if coord_term:
        Wy, Dy, ey = pos_taps_1d(g_old, gh)
        Wx, Dx, ex = pos_taps_1d(g_old, gw)
        g = p[1:].reshape(g_old, g_old, D)
        sy = torch.einsum("xb,ybd->yxd", Wx, torch.einsum("ya,abd->ybd", Dy, g).abs()) * ey[:, None, None]
        sx = torch.einsum("ya,axd->yxd", Wy, torch.einsum("xb,abd->axd", Dx, g).abs()) * ex[None, :, None]
        bound = bound + (sy + sx).reshape(gh * gw, D)
    return ref, torch.cat([torch.zeros(1, D, dtype=torch.float64), bound], 0)


def pos_weight_matrix(g_old, gh, gw, align_corners=False):
    """W [gh*gw, g_old^2] fp64 with resized = W @ grid: the resize of the unit images."""
    eye = torch.eye(g_old * g_old, dtype=torch.float64).reshape(g_old * g_old, 1, g_old, g_old)
    o = F.interpolate(eye, size=(gh, gw), mode="bilinear", align_corners=align_corners)
    return o.reshape(g_old * g_old, gh * gw).t().contiguous()


def pos_resize_backward_ref(dpos, posemb0, cls0, g_old, gh, gw, align_corners=False, coord_term=True):
    """fp64 autograd of pos_resize_ref added to the pre-filled posemb0 [1+g_old^2, D] / cls0 [D] (None: no dcls).
    Bound per element (n + 4) * 2^-24 * (|pre-fill| + sum|w dpos|), n = resized positions in that cell's footprint: per term one
    rounding each for 1-ly, 1-lx, wy*wx and the product with dpos (4; a weight clamped to the last cell is (1-l)+l, which rounds to
    exactly 1), then n - 1 inexact additions into the accumulator (the first lands on 0) and one into the destination (n); the
    pre-filled value is a term of that last addition, hence in the sum.  Row 0 and dcls are one fp32 addition each: 1 * 2^-24.  As in the forward, that count took the
    fraction to carry one rounding; it carries the fp32 source coordinate's absolute error (pos_taps_1d), so each weight wy * wx is
    off by up to dsrc_y |d wy| wx + wy dsrc_x |d wx|, and the bound adds the sum of that times |dpos| over the footprint."""
    D = dpos.shape[1]
    p = torch.zeros(1 + g_old * g_old, D, dtype=torch.float64, requires_grad=True)
    g = p[1:].reshape(1, g_old, g_old, D).permute(0, 3, 1, 2)
    o = F.interpolate(g, size=(gh, gw), mode="bilinear", align_corners=align_corners).permute(0, 2, 3, 1).reshape(gh * gw, D)
    torch.cat([p[:1], o], 0).backward(dpos.double())
    Wm = pos_weight_matrix(g_old, gh, gw, align_corners)
    n = torch.cat([torch.ones(1, dtype=torch.float64), (Wm > 0).sum(0).double()])[:, None]
    mag = torch.cat([dpos[:1].double().abs(), Wm.t() @ dpos[1:].double().abs()], 0) + posemb0.double().abs()
    ref = posemb0.double() + p.grad
    bound = (n + 4) * U24 * mag
    bound[0] = U24 * mag[0]
    if coord_term:
        Wy, Dy, ey = pos_taps_1d(g_old, gh)
        Wx, Dx, ex = pos_taps_1d(g_old, gw)
        a = dpos[1:].double().abs().reshape(gh, gw, D)
        c = (torch.einsum("ya,xb,yxd->abd", Dy.abs() * ey[:, None], Wx, a)
             + torch.einsum("ya,xb,yxd->abd", Wy, Dx.abs() * ex[:, None], a)).reshape(g_old * g_old, D)
        bound = bound + torch.cat([torch.zeros(1, D, dtype=torch.float64), c], 0)
    if cls0 is None:
        return ref, bound, None, None
    return ref, bound, cls0.double() + dpos[0].double(), U24 * (cls0.double().abs() + dpos[0].double().abs())


# ---- embedding / readout ------------------------------------------------------------------------------------------------------------------
def embed_backward_ref(gx, dtype, drop_last_image=False):
    """gx [B,ntok,D] fp32 -> dtok [B*np, D] `dtype` (one round-to-nearest-even, exact), dpos ref / bound: B - 1 inexact additions
    (b ascending, the first onto 0 is exact) <= B * 2^-24 * sum_b|gx|."""
    B, ntok, D = gx.shape
    src = gx[:-1] if drop_last_image else gx
    dtok = gx[:, 1:].to(dtype).reshape(B * (ntok - 1), D)
    return dtok, src.double().sum(0), B * U24 * gx.double().abs().sum(0)


def readout_cat_ref(x, dtype, swap_halves=False):
    B, ntok, D = x.shape
    a, b = x[:, 1:], x[:, :1].expand(-1, ntok - 1, -1)
    return torch.cat((b, a) if swap_halves else (a, b), -1).to(dtype).reshape(B * (ntok - 1), 2 * D)


def readout_cat_backward_ref(gx0, dcat, drop_last_patch=False):
    """gx0 [B,ntok,D] fp32 pre-fill, dcat [B*np, 2D] 16-bit -> (patch rows fp32, exact: one fp32 addition of two fp32 values is the
    same on every IEEE machine), (cls ref, bound).  cls: 32 interleaved lane sums over p, the 32 lanes in order, one addition into
    gx: at most np inexact additions on any path, inside (np + 1) * 2^-24 of |gx0| + sum_p|dcat|."""
    B, ntok, D = gx0.shape
    np_ = ntok - 1
    d = dcat.reshape(B, np_, 2 * D)
    patch = gx0[:, 1:] + d[..., :D].float()
    c = d[..., D:].double()
    cls = gx0[:, 0].double() + (c[:, :-1] if drop_last_patch else c).sum(1)
    bound = (np_ + 1) * U24 * (gx0[:, 0].double().abs() + c.abs().sum(1))
    return patch, cls, bound


# ---- 16-bit map permutations ------------------------------------------------------------------------------------------------------------------
def unpad_rows_ref(xpad, off=1):
    B, Hp, Wp, C = xpad.shape
    H, W = Hp - 2, Wp - 2
    return xpad[:, off:off + H, off:off + W].reshape(B * H * W, C).clone()


def dilate2_ref(dypad, H, W, start=1):
    """dypad [B,Ho+2,Wo+2,C] -> [B,H+2,W+2,C], zero except dyd[2y+1, 2x+1] = dy[y+1, x+1] (padded coordinates)."""
    B, Hop, Wop, C = dypad.shape
    out = torch.zeros((B, H + 2, W + 2, C), dtype=dypad.dtype)
    out[:, start:start + 2 * (Hop - 2):2, start:start + 2 * (Wop - 2):2] = dypad[:, 1:-1, 1:-1]
    return out


def unpixshuf_ref(dl, gh, gw, s, swap_ij=False):
    """dl padded [B,gh*s+2,gw*s+2,C] -> [B*gh*gw, s*s*C], column (i*s+j)*C + c = dl[b, y*s+i+1, x*s+j+1, c]."""
    B, C = dl.shape[0], dl.shape[-1]
    v = dl[:, 1:-1, 1:-1].reshape(B, gh, s, gw, s, C)                       # b y i x j c
    v = v.permute(0, 1, 3, 4, 2, 5) if swap_ij else v.permute(0, 1, 3, 2, 4, 5)
    return v.reshape(B * gh * gw, s * s * C).clone()


# ---- ConvTranspose2d(kernel = stride = s) as a GEMM on rows (lseg_vit.py:457-466) ---------------------------------------------------------
def pack_convT_ref(w, Cp, s, dtype, fill, swap_ij=False):
    """w [Ci,Co,s,s] fp32 -> [(i*s+j)*Cp + co, Cp(ci)] `dtype`; entries outside Ci x Co keep `fill` (the kernel leaves them alone)."""
    Ci, Co = w.shape[:2]
    out = fill.clone().reshape(s, s, Cp, Cp)
    out[:, :, :Co, :Ci] = (w.permute(3, 2, 1, 0) if swap_ij else w.permute(2, 3, 1, 0)).to(dtype)
    return out.reshape(s * s * Cp, Cp)


def check_convT_forward(fwd, want, C, name):
    """The packed weight times the rows, through the pixel-shuffle indexing, is F.conv_transpose2d (fp64 on both sides: products of
    16-bit values summed in another order, 1e-12 relative) and nothing lands in the padded output channels."""
    assert_max_err(fwd[:, :C], want, 1e-12 * want.abs().max().item(), name)
    assert not fwd[:, C:].any(), f"{name}: padded output channels are not zero"


def convT_forward_from_packed(rows, wp, B, gh, gw, s, Cp):
    """rows [B*gh*gw, Cp] x packed weight -> NCHW [B,Cp,gh*s,gw*s] through the pixel-shuffle indexing, fp64."""
    y = rows.double() @ wp.double().t()                                         # [M, (i*s+j)*Cp + co]
    return y.reshape(B, gh, gw, s, s, Cp).permute(0, 5, 1, 3, 2, 4).reshape(B, Cp, gh * s, gw * s)


def convT_wgrad_unpack_ref(dw, C, Cp, s, swap_ij=False):
    """dw [(i*s+j)*Cp + co, Cp(ci)] -> [ci, co, i, j] over the real C x C channels."""
    v = dw.reshape(s, s, Cp, Cp)[:, :, :C, :C]                                  # i j co ci
    return (v.permute(3, 2, 1, 0) if swap_ij else v.permute(3, 2, 0, 1)).contiguous()


def convT_backward_autograd(x, w, b, dL, s):
    """fp64 autograd of F.conv_transpose2d(x, w, b, stride=s) for d(out) = dL: (dw [C,C,s,s], db [C])."""
    wr, br = w.double().requires_grad_(True), b.double().requires_grad_(True)
    F.conv_transpose2d(x.double(), wr, br, stride=s).backward(dL.double())
    return wr.grad, br.grad


def check_convT_grads(dw, db, ref_dw, ref_db, name):
    """test_linear_backward's bars for dw and db (fp32 accumulation order only)."""
    assert_max_err(dw, ref_dw, 2e-4 * ref_dw.abs().max().item() + 1e-6, name + ".dw")
    assert_max_err(db, ref_db, 2e-4 * max(1.0, ref_db.abs().max().item()), name + ".db")


def conv_s2_backward_autograd(x, w, dy):
    xr, wr = x.double().requires_grad_(True), w.double().requires_grad_(True)
    F.conv2d(xr, wr, None, stride=2, padding=1).backward(dy.double())
    return xr.grad, wr.grad


def check_conv_s2_grads(dx, dw, ref_dx, ref_dw, name):
    """test_conv3x3_backward's bars."""
    assert_max_err(dx, ref_dx, 2e-2 * max(1.0, ref_dx.abs().max().item()), name + ".dx")
    assert_max_err(dw, ref_dw, 2e-3 * max(1.0, ref_dw.abs().max().item()), name + ".dw")


# ---- fp32 partial sums ----------------------------------------------------------------------------------------------------------------------
def _sum_ref(terms, prefill):
    """terms [T, ...] fp32 summed in order (+ prefill): T - 1 inexact additions (the first lands on 0 or is the initial value) plus one
    for the pre-fill, <= (terms + 1) * 2^-24 * sum|terms| with the pre-fill counted as a term."""
    t = terms.double()
    ref, mag, k = t.sum(0), t.abs().sum(0), terms.shape[0]
    if prefill is not None:
        ref, mag, k = ref + prefill.double(), mag + prefill.double().abs(), k + 1
    return ref, (k + 1) * U24 * mag, k


def conv_wgrad_unpack_ref(slabs, Co, Ci, prefill=None, drop_slab=False):
    """slabs [nsplit, Co_p, 9, Cip] fp32 (tap-major) -> OIHW [Co,Ci,3,3]: (ref, bound, number of terms)."""
    v = slabs[:, :Co, :, :Ci].permute(0, 1, 3, 2).reshape(slabs.shape[0], Co, Ci, 3, 3)
    return _sum_ref(v[:-1] if drop_slab else v, prefill)


def sum_partials_ref(part, n, prefill=None, drop_slab=False):
    """part [nsplit, stride] fp32 -> [n]."""
    v = part[:, :n]
    return _sum_ref(v[:-1] if drop_slab else v, prefill)


def fold_rows_ref(src, C, prefill=None, drop_row=False):
    """src [R, ld] fp32 -> [C]."""
    v = src[:, :C]
    return _sum_ref(v[:-1] if drop_row else v, prefill)


# ---- BatchNorm running statistics -------------------------------------------------------------------------------------------------------
def bn_running_ref(x, rmean0, rvar0, momentum=0.1, biased=False):
    """x [count, C] fp64 samples -> (stats [2C] fp32 = {sum x, sum x^2} as the kernel receives them, new rmean, its bound, new rvar,
    its bound) from one train-mode forward of nn.BatchNorm2d(C, momentum) in fp64.
    mean: the new term passes 6 roundings (sum x to fp32, 1/n, their product, momentum to fp32, its product, the addition) and is
    scaled by momentum = 0.1: 0.6 * 2^-24 |mean|; the old term passes 3 (1 - momentum, its product with rmean, the addition) scaled
    by 0.9: 2.7 * 2^-24 |rmean|; both inside 4 * 2^-24 * (|rmean| + |mean|).  var: E[x^2] - mean^2 is formed in fp32, so its
    cancellation error scales with sum x^2 / n + mean^2, not with var.  sum x^2 / n passes 9 roundings (to fp32, 1/n, product, the
    subtraction, momentum, its product, count/(count-1), its product, the addition), mean^2 passes 13 (3 in each factor, the square,
    then the same 6), scaled by momentum * count/(count-1) <= 0.2: 2.6 * 2^-24; rvar as rmean: 2.7 * 2^-24; both inside
    8 * 2^-24 * (|rvar| + sum x^2 / n + mean^2).
    count == 1 has no unbiased variance (torch refuses the forward): launch_bn_running_update then uses the biased one, which is 0."""
    count, C = x.shape
    stats = torch.cat([x.sum(0), (x * x).sum(0)]).float()
    mean, ex2 = x.mean(0), (x * x).mean(0)
    if count > 1 and not biased:
        bn = torch.nn.BatchNorm2d(C, momentum=momentum).double().train()
        with torch.no_grad():
            bn.running_mean.copy_(rmean0.double())
            bn.running_var.copy_(rvar0.double())
            bn(x.reshape(count, C, 1, 1))
        rm, rv = bn.running_mean.clone(), bn.running_var.clone()
    else:
        rm = (1 - momentum) * rmean0.double() + momentum * mean
        rv = (1 - momentum) * rvar0.double() + momentum * x.var(0, unbiased=False)
    return (stats, rm, 4 * U24 * (rmean0.double().abs() + mean.abs()),
            rv, 8 * U24 * (rvar0.double().abs() + ex2 + mean * mean))
