"""Host-side self-check of tests/glue_helpers.py: for every reference the GPU test uses, a plain fp32 torch emulation of the kernel's
arithmetic passes the comparison and a deliberately wrong variant fails it -- through the same comparison functions
tests/test_gpu_train_glue.py calls.  This is what shows the bars are tight enough to see a wrong clamp, a dropped row or a swapped
(i, j); it needs no GPU."""
import pytest
import torch

import glue_helpers as G

BF, FP = torch.bfloat16, torch.float16


def rejected(fn, *a):
    with pytest.raises(AssertionError):
        fn(*a)


def _taps_f32(n_in, n_out, coord="fp32"):
    """One axis of the resize kernels' taps in fp32 on the host: (i0, i1, l).  "fp32": PyTorch's fp32 formula, as the kernels compute
    it; "exact": the rational ((2i+1) n_in - n_out) / (2 n_out) with one rounding for its fraction; "fp16_scale": a wrong kernel whose
    scale n_in / n_out went through a 16-bit register."""
    f32 = torch.float32
    i = torch.arange(n_out)
    if coord == "exact":
        num = ((2 * i + 1) * n_in - n_out).clamp(min=0)
        i0 = num // (2 * n_out)
        l = (num - i0 * 2 * n_out).to(f32) / torch.tensor(2.0 * n_out, dtype=f32)
    else:
        r = torch.tensor(float(n_in), dtype=f32) / torch.tensor(float(n_out), dtype=f32)
        if coord == "fp16_scale":
            r = r.half().float()
        s = ((i.to(f32) + 0.5) * r - 0.5).clamp(min=0)
        i0 = s.to(torch.int64)
        l = s - i0.to(f32)
    return i0, i0 + (i0 < n_in - 1).long(), l


def _resize_f32(pos, g_old, gh, gw, coord="fp32"):
    """pos_resize_kernel's arithmetic in fp32 on the host."""
    y0, y1, ly = _taps_f32(g_old, gh, coord)
    x0, x1, lx = _taps_f32(g_old, gw, coord)
    g = pos[1:].reshape(g_old, g_old, -1)
    ly, lx = ly[:, None, None], lx[None, :, None]
    top = (1 - lx) * g[y0][:, x0] + lx * g[y0][:, x1]
    bot = (1 - lx) * g[y1][:, x0] + lx * g[y1][:, x1]
    out = (1 - ly) * top + ly * bot
    return torch.cat([pos[:1], out.reshape(gh * gw, -1)], 0)


def _resize_bwd_f32(dpos, pe0, g_old, gh, gw, coord="fp32"):
    """pos_resize_bwd_kernel's weights in fp32 on the host (the sum runs in another order: still inside the counted bound)."""
    def w1d(n_out):
        i0, i1, l = _taps_f32(g_old, n_out, coord)
        w = torch.zeros(n_out, g_old)
        r = torch.arange(n_out)
        w[r, i0] += 1 - l
        w[r, i1] += l
        return w
    acc = torch.einsum("ya,xb,yxd->abd", w1d(gh), w1d(gw), dpos[1:].reshape(gh, gw, -1))
    return pe0 + torch.cat([dpos[:1], acc.reshape(g_old * g_old, -1)], 0)


POS_SHAPES = [(24, 30, 30, 64), (24, 6, 10, 64), (4, 7, 3, 8), (2, 2, 5, 8)]


@pytest.mark.parametrize("g_old,gh,gw,D", POS_SHAPES)
def test_pos_resize_bar(g_old, gh, gw, D):
    pos = G.randn((1 + g_old * g_old, D), 1)
    ref, bound = G.pos_resize_ref(pos, g_old, gh, gw)
    G.assert_within(_resize_f32(pos, g_old, gh, gw), ref, bound, "host.pos_resize")
    G.assert_within(_resize_f32(pos, g_old, gh, gw, "exact"), ref, bound, "host.pos_resize.exact_coordinate")
    wrong, _ = G.pos_resize_ref(pos, g_old, gh, gw, align_corners=True)
    rejected(G.assert_within, wrong.float(), ref, bound, "host.pos_resize.align_corners")
    last_row = _resize_f32(pos, g_old, gh, gw)
    last_row[-gw:] = last_row[-2 * gw:-gw] if gh > 1 else 0          # the last output row takes the taps of the one above
    rejected(G.assert_within, last_row, ref, bound, "host.pos_resize.last_row")
    rejected(G.assert_within, _resize_f32(pos, g_old, gh, gw, "fp16_scale"), ref, bound, "host.pos_resize.fp16_scale")


def test_pos_resize_first_count_missed_the_coordinate_magnitude():
    """24 -> 30 (the 480 x 480 case).  Without the coordinate term the bar is 8 * 2^-24 * sum|w v|, which allows the fraction one
    rounding.  PyTorch's fp32 coordinate, which the kernels reproduce, is rounded at the magnitude of the grid index (up to 2^-20
    absolute at index 16..31) and the fraction inherits that: a correct kernel misses the first count, a kernel with an exact
    rational coordinate meets it.  The recounted bar (pos_taps_1d) holds for both and still rejects a 16-bit scale (above)."""
    pos = G.randn((1 + 24 * 24, 64), 1)
    ref, first = G.pos_resize_ref(pos, 24, 30, 30, coord_term=False)
    rejected(G.assert_within, _resize_f32(pos, 24, 30, 30), ref, first, "host.pos_resize.first_count")
    G.assert_within(_resize_f32(pos, 24, 30, 30, "exact"), ref, first, "host.pos_resize.first_count.exact_coordinate")


@pytest.mark.parametrize("g_old,gh,gw,D", POS_SHAPES)
def test_pos_resize_backward_bar(g_old, gh, gw, D):
    dpos = G.randn((1 + gh * gw, D), 2)
    pe0, cls0 = G.randn((1 + g_old * g_old, D), 3), G.randn((D,), 4)
    ref, bound, rcls, bcls = G.pos_resize_backward_ref(dpos, pe0, cls0, g_old, gh, gw)
    emu = _resize_bwd_f32(dpos, pe0, g_old, gh, gw)
    G.assert_within(emu, ref, bound, "host.pos_resize_backward")
    G.assert_within(_resize_bwd_f32(dpos, pe0, g_old, gh, gw, "exact"), ref, bound, "host.pos_resize_backward.exact_coordinate")
    G.assert_within(cls0 + dpos[0], rcls, bcls, "host.pos_resize_backward.cls")
    wrong, _, _, _ = G.pos_resize_backward_ref(dpos, pe0, cls0, g_old, gh, gw, align_corners=True)
    rejected(G.assert_within, wrong.float(), ref, bound, "host.pos_resize_backward.align_corners")
    rejected(G.assert_within, emu - pe0, ref, bound, "host.pos_resize_backward.overwrites")          # = instead of +=
    rejected(G.assert_within, _resize_bwd_f32(dpos, pe0, g_old, gh, gw, "fp16_scale"), ref, bound, "host.pos_resize_backward.fp16_scale")
    # the adjoint identity on the references themselves (what the GPU test asserts of the kernels' outputs to 1e-5)
    p, q = G.randn((1 + g_old * g_old, D), 5), dpos
    fwd, _ = G.pos_resize_ref(p, g_old, gh, gw)
    bwd, _, _, _ = G.pos_resize_backward_ref(q, torch.zeros_like(pe0), None, g_old, gh, gw)
    lhs, rhs = (fwd * q.double()).sum().item(), (p.double() * bwd).sum().item()
    assert abs(lhs - rhs) <= 1e-12 * max(abs(lhs), abs(rhs), 1.0)
    bad, _ = G.pos_resize_ref(p, g_old, gh, gw, align_corners=True)                                    # a pair on different taps
    assert abs((bad * q.double()).sum().item() - rhs) > 1e-5 * max(abs(lhs), abs(rhs))


@pytest.mark.parametrize("dtype", [BF, FP])
@pytest.mark.parametrize("B,ntok,D", [(1, 5, 8), (3, 37, 192), (8, 10, 64)])
def test_embed_backward_bar(B, ntok, D, dtype):
    gx = G.randn((B, ntok, D), 6)
    dtok, dpos, bound = G.embed_backward_ref(gx, dtype)
    G.assert_bits_equal(gx[:, 1:].to(dtype).reshape(-1, D), dtok, "host.embed_backward.dtok")
    G.assert_within(gx.sum(0), dpos, bound, "host.embed_backward.dpos")
    rejected(G.assert_bits_equal, gx[:, :-1].to(dtype).reshape(-1, D), dtok, "host.embed_backward.dtok.cls_row_kept")
    trunc = (gx[:, 1:].contiguous().view(torch.int32) >> 16 << 16).view(torch.float32).to(dtype).reshape(-1, D)
    rejected(G.assert_bits_equal, trunc, dtok, "host.embed_backward.dtok.truncated")                 # round toward zero
    if B > 1:
        _, wrong, _ = G.embed_backward_ref(gx, dtype, drop_last_image=True)
        rejected(G.assert_within, wrong.float(), dpos, bound, "host.embed_backward.dpos.image_dropped")


@pytest.mark.parametrize("dtype", [BF, FP])
@pytest.mark.parametrize("B,ntok,D", [(2, 37, 192), (1, 2, 8), (3, 65, 256), (1, 34, 264)])
def test_readout_bars(B, ntok, D, dtype):
    x = G.randn((B, ntok, D), 7)
    ref = G.readout_cat_ref(x, dtype)
    rejected(G.assert_bits_equal, G.readout_cat_ref(x, dtype, swap_halves=True), ref, "host.readout_cat.swapped")
    gx0, dcat = G.randn((B, ntok, D), 8), G.randn((B * (ntok - 1), 2 * D), 9, 0.5, dtype)
    patch, cls, bound = G.readout_cat_backward_ref(gx0, dcat)
    emu = gx0[:, 0] + dcat.float().reshape(B, ntok - 1, 2 * D)[..., D:].sum(1)
    G.assert_within(emu, cls, bound, "host.readout_cat_backward.cls")
    _, wrong, _ = G.readout_cat_backward_ref(gx0, dcat, drop_last_patch=True)
    rejected(G.assert_within, wrong.float(), cls, bound, "host.readout_cat_backward.cls.last_patch_dropped")
    rejected(G.assert_bits_equal, dcat.float().reshape(B, ntok - 1, 2 * D)[..., :D].contiguous(), patch, "host.readout_cat_backward.overwrites")


def test_permutation_bars():
    x = G.with_specials16(G.randn((2, 7, 9, 8), 10, dtype=BF))
    ref = G.unpad_rows_ref(x)
    G.assert_bits_equal(x[:, 1:-1, 1:-1].reshape(-1, 8), ref, "host.unpad_rows")
    rejected(G.assert_bits_equal, G.unpad_rows_ref(x, off=0), ref, "host.unpad_rows.border_kept")
    for H, W in ((15, 15), (30, 16), (2, 3)):
        dy = G.with_specials16(G.randn((1, (H - 1) // 2 + 3, (W - 1) // 2 + 3, 8), 11, dtype=BF))
        ref = G.dilate2_ref(dy, H, W)
        assert ref[:, 0].abs().max() == 0 and ref[:, :, 0].abs().max() == 0 and ref[:, 2::2].abs().max() == 0
        rejected(G.assert_bits_equal, G.dilate2_ref(dy, H, W, start=0), ref, "host.dilate2.off_by_one")
    neg0 = torch.zeros((1, 3, 3, 8), dtype=BF)
    neg0.view(torch.int16)[0, 1, 1, 0] = -0x8000
    rejected(G.assert_bits_equal, torch.zeros((1, 4, 4, 8), dtype=BF), G.dilate2_ref(neg0, 2, 2), "host.dilate2.negative_zero_lost")
    dl = G.with_specials16(G.randn((2, 3 * 4 + 2, 5 * 4 + 2, 8), 12, dtype=FP))
    ref = G.unpixshuf_ref(dl, 3, 5, 4)
    rejected(G.assert_bits_equal, G.unpixshuf_ref(dl, 3, 5, 4, swap_ij=True), ref, "host.unpixshuf.ij_swapped")


@pytest.mark.parametrize("B,gh,gw,C,Cp,s", [(1, 3, 5, 48, 64, 4), (2, 4, 4, 64, 64, 2)])
def test_convT_composed_bar(B, gh, gw, C, Cp, s):
    """The ConvTranspose backward as the engine composes it (unpixshuf -> GEMM wgrad -> unpack + fold), in fp64 torch on the helpers'
    layouts, against autograd: right layout accepted, (i, j) swapped rejected, padded channels reaching the result rejected."""
    x = G.randn((B, C, gh, gw), 13, dtype=BF).float()
    w = G.randn((C, C, s, s), 14, C ** -0.5, BF).float()
    b = G.randn((C,), 15)
    dL = G.randn((B, C, gh * s, gw * s), 16, 0.5, BF).float()
    ref_dw, ref_db = G.convT_backward_autograd(x, w, b, dL, s)
    rows = G.randn((B * gh * gw, Cp), 17)                                       # padded columns: finite garbage
    rows[:, :C] = x.permute(0, 2, 3, 1).reshape(-1, C)
    dl = G.randn((B, gh * s + 2, gw * s + 2, Cp), 18)                           # border and padded channels: finite garbage
    dl[:, 1:-1, 1:-1, :C] = dL.permute(0, 2, 3, 1)
    zeros = torch.zeros(s * s * Cp, Cp)
    wp = G.pack_convT_ref(w, Cp, s, torch.float32, zeros)
    clean = torch.cat([rows[:, :C], torch.zeros(rows.shape[0], Cp - C)], 1)
    want = torch.nn.functional.conv_transpose2d(x.double(), w.double(), None, stride=s)
    G.check_convT_forward(G.convT_forward_from_packed(clean, wp, B, gh, gw, s, Cp), want, C, "host.pack_convT.forward")
    swapped = G.pack_convT_ref(w, Cp, s, torch.float32, zeros, swap_ij=True)                 # (i, j) swapped in the pack
    rejected(G.assert_bits_equal, swapped, wp, "host.pack_convT.ij_swapped")
    rejected(G.check_convT_forward, G.convT_forward_from_packed(clean, swapped, B, gh, gw, s, Cp), want, C, "host.pack_convT.forward.ij_swapped")
    if Cp > C:                                                                               # a pack that writes (zeroes) the padding
        pattern = G.randn((s * s * Cp, Cp), 22)
        rejected(G.assert_bits_equal, wp, G.pack_convT_ref(w, Cp, s, torch.float32, pattern), "host.pack_convT.padding_written")
        leaky = G.pack_convT_ref(w, Cp, s, torch.float32, pattern)                           # padding left non-zero reaches the output
        rejected(G.check_convT_forward, G.convT_forward_from_packed(rows, leaky, B, gh, gw, s, Cp), want, C, "host.pack_convT.forward.padding")
    dG = G.unpixshuf_ref(dl, gh, gw, s).double()
    dw_gemm, db_gemm = dG.t() @ rows.double(), dG.sum(0)
    dw = G.convT_wgrad_unpack_ref(dw_gemm, C, Cp, s)
    db, _, _ = G.fold_rows_ref(db_gemm.reshape(s * s, Cp).float(), C)
    G.check_convT_grads(dw, db, ref_dw, ref_db, "host.convT")
    rejected(G.check_convT_grads, G.convT_wgrad_unpack_ref(dw_gemm, C, Cp, s, swap_ij=True), db, ref_dw, ref_db, "host.convT.ij_swapped")
    if Cp > C:
        shifted = dw_gemm.reshape(s, s, Cp, Cp)[:, :, Cp - C:, :C].permute(3, 2, 0, 1)             # reads the padded rows
        rejected(G.check_convT_grads, shifted, db, ref_dw, ref_db, "host.convT.padded_rows")
    short, _, _ = G.fold_rows_ref(db_gemm.reshape(s * s, Cp).float(), C, drop_row=True)
    rejected(G.check_convT_grads, dw, short, ref_dw, ref_db, "host.convT.bias_group_dropped")


def test_conv_s2_composed_bar():
    """Stride-2 conv backward = stride-1 backward on the dilated gradient: accepted; with the dilation off by one: rejected."""
    import torch.nn.functional as F
    B, H, W, Ci, Co = 1, 15, 15, 64, 64
    x = G.randn((B, Ci, H, W), 19, dtype=BF).float()
    w = G.randn((Co, Ci, 3, 3), 20, (9 * Ci) ** -0.5, BF).float()
    dy = G.randn((B, Co, 8, 8), 21, dtype=BF).float()
    ref_dx, ref_dw = G.conv_s2_backward_autograd(x, w, dy)
    dyp = torch.zeros((B, 10, 10, Co))
    dyp[:, 1:-1, 1:-1] = dy.permute(0, 2, 3, 1)
    for start, ok in ((1, True), (2, False)):
        dyd = G.dilate2_ref(dyp, H, W, start=start)[:, 1:-1, 1:-1].permute(0, 3, 1, 2).double()
        xr, wr = x.double().requires_grad_(True), w.double().requires_grad_(True)
        F.conv2d(xr, wr, None, stride=1, padding=1).backward(dyd)
        if ok:
            G.check_conv_s2_grads(xr.grad, wr.grad, ref_dx, ref_dw, "host.conv_s2")
        else:
            rejected(G.check_conv_s2_grads, xr.grad, wr.grad, ref_dx, ref_dw, "host.conv_s2.off_by_one")


@pytest.mark.parametrize("acc", [0, 1])
def test_partial_sum_bars(acc):
    for Co, Ci, Cip, ns in ((5, 3, 8, 1), (64, 48, 64, 3), (8, 8, 8, 8)):
        slabs = G.randn((ns, Co + 3, 9, Cip), 22)
        pre = G.randn((Co, Ci, 3, 3), 23) if acc else None
        ref, bound, _ = G.conv_wgrad_unpack_ref(slabs, Co, Ci, pre)
        emu = slabs[:, :Co, :, :Ci].permute(0, 1, 3, 2).sum(0).reshape(Co, Ci, 3, 3) + (pre if acc else 0)
        G.assert_within(emu, ref, bound, "host.conv_wgrad_unpack")
        if ns > 1:
            wrong, _, _ = G.conv_wgrad_unpack_ref(slabs, Co, Ci, pre, drop_slab=True)
            rejected(G.assert_within, wrong.float(), ref, bound, "host.conv_wgrad_unpack.slab_dropped")
        tapmajor = slabs[:, :Co, :, :Ci].sum(0).reshape(Co, Ci, 3, 3) + (pre if acc else 0)          # no tap-major -> OIHW re-layout
        rejected(G.assert_within, tapmajor, ref, bound, "host.conv_wgrad_unpack.not_relaid")
    for ns, n in ((1, 4), (5, 4 * 1031), (8, 4096)):
        part = G.randn((ns, n + 8), 24)
        pre = G.randn((n,), 25) if acc else None
        ref, bound, _ = G.sum_partials_ref(part, n, pre)
        G.assert_within(part[:, :n].sum(0) + (pre if acc else 0), ref, bound, "host.sum_partials")
        if ns > 1:
            wrong, _, _ = G.sum_partials_ref(part, n, pre, drop_slab=True)
            rejected(G.assert_within, wrong.float(), ref, bound, "host.sum_partials.slab_dropped")
        if acc:
            rejected(G.assert_within, part[:, :n].sum(0), ref, bound, "host.sum_partials.overwrites")
    for R, C_, ld in ((1, 64, 64), (16, 48, 64), (4, 300, 320)):
        src = G.randn((R, ld), 26)
        pre = G.randn((C_,), 27) if acc else None
        ref, bound, _ = G.fold_rows_ref(src, C_, pre)
        G.assert_within(src[:, :C_].sum(0) + (pre if acc else 0), ref, bound, "host.fold_rows")
        if R > 1:
            wrong, _, _ = G.fold_rows_ref(src, C_, pre, drop_row=True)
            rejected(G.assert_within, wrong.float(), ref, bound, "host.fold_rows.row_dropped")


@pytest.mark.parametrize("C_,count", [(8, 2), (64, 450), (300, 7200), (8, 1)])
def test_bn_running_bar(C_, count):
    x = G.randn((count, C_), 28, 0.5, torch.float64) + 1.5
    rm0, rv0 = G.randn((C_,), 29), G.randn((C_,), 30).abs() + 0.5
    stats, rm, bm, rv, bv = G.bn_running_ref(x, rm0, rv0)
    inv_n = torch.tensor(1.0 / count, dtype=torch.float32)
    mean = stats[:C_] * inv_n
    var = (stats[C_:] * inv_n - mean * mean).clamp(min=0)
    unb = torch.tensor(count / (count - 1.0) if count > 1 else 1.0, dtype=torch.float32)
    m = torch.tensor(0.1, dtype=torch.float32)
    G.assert_within((1 - m) * rm0 + m * mean, rm, bm, "host.bn_running.mean")
    G.assert_within((1 - m) * rv0 + m * var * unb, rv, bv, "host.bn_running.var")
    if count > 1:
        _, _, _, wrong, _ = G.bn_running_ref(x, rm0, rv0, biased=True)
        rejected(G.assert_within, wrong.float(), rv, bv, "host.bn_running.var.biased")
        rejected(G.assert_within, (0.1 * mean).float(), rm, bm, "host.bn_running.mean.overwrites")
    else:
        assert torch.equal(rv, 0.9 * rv0.double())                      # the documented count == 1 form: biased variance, which is 0
