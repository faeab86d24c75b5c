"""Host-side self-check of tests/tail_helpers.py: for every reference tests/test_gpu_output_tail.py uses, a plain fp32 torch emulation of
the kernel's arithmetic passes the comparison and a deliberately wrong variant fails it -- through the same comparison functions -- and
the inputs of every GPU case meet the 1 % cap on widened fp16 intervals from the reference alone.  Needs no GPU."""
import pytest
import torch

import tail_helpers as T

F32 = torch.float32


def rejected(what, fn, *a, **kw):
    with pytest.raises(AssertionError) as e:
        fn(*a, **kw)
    print(f"wrong-variant {what}: {str(e.value).splitlines()[0]}")


def test_last_output_index_lands_on_the_last_cell_in_fp32():
    """src_tap at i = 2n-1: fl(fl((n-1) / (2n-1)) * (2n-1)) == n-1 for every n in 2..1100, so the last row / column has l = 0, both taps
    on the last cell and no coordinate term."""
    n = torch.arange(2, 1101).to(F32)
    r = (n - 1) / (2 * n - 1)
    assert torch.equal(r * (2 * n - 1), n - 1)
    for k in (2, 3, 17, 258, 1100):
        i0, i1, l = T.taps_f32(k)
        assert i0[-1] == k - 1 and i1[-1] == k - 1 and l[-1] == 0 and (l >= 0).all() and (l < 1).all()
        j0, j1, _, _, _, _ = T.ac_taps(k)
        assert torch.equal(i0, j0) and torch.equal(i1, j1), "an fp32 tap differs from the fp64 one"


def test_numpy_rounds_a_double_to_fp16_once():
    x = torch.tensor([1 + 2.0 ** -11 + 2.0 ** -30], dtype=torch.float64)
    lo, _ = T.f16_ends(x, torch.zeros_like(x))
    assert lo.item() == 1 + 2.0 ** -10


# ---- a. gram ----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,H,W,C", T.GRAM_SHAPES)
def test_gram_bar(B, H, W, C):
    g = T.feature_map(B, H, W, C, 10 + C, None, torch.float16)
    ref, mag = T.gram_ref(g)
    bound = T.gram_bound(mag, C)
    T.assert_within(T.emu_gram(g), ref, bound, "host.pixel_gram")
    if H * W > 1:
        rejected("gram: diag / anti swapped", T.assert_within, T.emu_gram(g, swap_diag_anti=True), ref, bound, "host.pixel_gram.swapped")
    zero_border = g.clone()
    zero_border[:, -1] = 0                                       # a kernel that did not read the padded row below the last one
    rejected("gram: border row not read", T.assert_within, T.emu_gram(zero_border), ref, bound, "host.pixel_gram.border")


# ---- b. norm plane ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rough", [0.1, None])
@pytest.mark.parametrize("B,H,W", T.NORM_SHAPES)
def test_norm_plane_bar(B, H, W, rough):
    g = T.feature_map(B, H, W, 64, 20 + H, rough, torch.float16)
    gram32, ref, bound, n2, form = T.norm_plane_ref(g, T.LOGIT_SCALE)
    assert ((form - n2).abs() <= 1e-12 * n2).all(), "the reference's quadratic form is not ||bilinear(g)||^2"
    tag = "smooth" if rough else "rough"
    T.assert_within(T.emu_norm_plane(gram32, H, W, T.LOGIT_SCALE), ref, bound, f"host.norm_scale_plane.{tag}")
    rejected(f"norm plane ({tag}): b.c / b.d swapped", T.assert_within, T.emu_norm_plane(gram32, H, W, T.LOGIT_SCALE, swap_bc_bd=True), ref, bound,
             "host.norm_scale_plane.swapped")
    rejected(f"norm plane ({tag}): cross terms not doubled", T.assert_within, T.emu_norm_plane(gram32, H, W, T.LOGIT_SCALE, cross=1.0), ref, bound,
             "host.norm_scale_plane.cross1")


def test_norm_plane_clamped_tap_must_weigh_nothing():
    """The kernel as first compiled: the fraction fused into fma(r, i, -i0).  At 30 -> 60 the last column gets lx = -7e-7 on a tap whose
    records are the pixel's own, so a.(border column) enters its norm: with independent neighbours that misses the counted bound (1.53 on
    the MI355X, the same here), with neighbours that share a direction the two misplaced terms cancel and it hides at 0.3."""
    B, H, W = 2, 17, 30
    assert T.taps_f32(W, fused=True)[2][-1] != 0 and T.taps_f32(W)[2][-1] == 0
    g = T.feature_map(B, H, W, 64, 20 + H, None, torch.float16)
    gram32, ref, bound, _, _ = T.norm_plane_ref(g, T.LOGIT_SCALE)
    rejected("norm plane (rough): fraction fused, clamped tap weighs 1e-6", T.assert_within,
             T.emu_norm_plane(gram32, H, W, T.LOGIT_SCALE, fused=True), ref, bound, "host.norm_scale_plane.fused_fraction")


def test_norm_plane_footprint():
    fp = T.footprint(3, 7, 1, 2)
    (y0, y1, x0, x1), w = T._cell_weights(3, 7)
    assert fp.sum().item() > 0 and fp.shape == (6, 14)
    # every output pixel that gives the record a non-zero weight lies inside it
    wsum = torch.zeros(6, 14, dtype=torch.float64)
    for yy, xx, ww in ((y0, x0, w[0]), (y0, x1, w[1]), (y1, x0, w[2]), (y1, x1, w[3])):
        wsum += ww * ((yy == 1)[:, None] & (xx == 2)[None, :])
    assert not (wsum[~fp] != 0).any()


# ---- c. scaled x2 / one-pass x4 ------------------------------------------------------------------------------------------------------------------
def _triple(R, scale, K, **kw):
    low = T.emu_low(R, scale, K, **kw)
    out = T.emu_bilerp(low)
    return low, out, out.clone()


@pytest.mark.parametrize("B,K,H,W", T.X4_SHAPES)
def test_x4_tail_bar(B, K, H, W):
    R, scale = T.x4_inputs(B, K, H, W)
    case = f"{B},{K},{H},{W}"
    low, out, one = _triple(R, scale, K)
    T.check_x4_tail(low, out, one, R, scale, K, case, who="host.upsample4x")
    chk = lambda what, *t: rejected(f"x4 [{case}]: {what}", T.check_x4_tail, *t, R, scale, K, case, who="host.upsample4x.wrong")
    chk("align_corners=False taps", *_triple(R, scale, K, align_corners=False))
    raw = T.emu_low(R, scale, K, round16=False)
    chk("fp16 rounding dropped (both forms)", raw, T.emu_bilerp(raw), T.emu_bilerp(raw))
    chk("fp16 rounding dropped (one pass)", low, out, T.emu_bilerp(raw))
    chk("fp16 rounding after the second x2 (one pass)", low, out, T.emu_bilerp(raw).half().float())
    if B > 1:
        chk("image 0's scale plane for every image", *_triple(R, scale, K, image0_scale=True))
        chk("image 0's scale plane for every image (one pass)", low, out, T.emu_bilerp(T.emu_low(R, scale, K, image0_scale=True)))
    if 2 * H > 16:                                               # a second band: its first output row from the source rows one above
        y0, y1, ly = T.taps_f32(2 * H)
        first = int((y0 >= 16).nonzero()[0])
        y0, y1 = y0.clone(), y1.clone()
        y0[first] -= 1
        y1[first] -= 1
        chk("a band's first row from the previous band's last source row (one pass)", low, out, T.emu_bilerp(low, ytaps=(y0, y1, ly)))
    stage2 = T.emu_bilerp(low, align_corners=False)
    chk("output_conv's x2 with align_corners=False (both forms)", low, stage2, stage2)


@pytest.mark.parametrize("P,H,W", T.X2_SHAPES)
def test_x2_planes_bar(P, H, W):
    v = T.randn((P, H, W), 50 + H)
    ref, bound = T.up2_planes_ref(v)
    T.assert_within(T.emu_bilerp(v), ref, bound, "host.upsample2x_planes")
    rejected("x2 planes: align_corners=False", T.assert_within, T.emu_bilerp(v, align_corners=False), ref, bound, "host.upsample2x_planes.ac")
    y0, y1, ly = T.taps_f32(H)
    rejected("x2 planes: last row from the row above", T.assert_within, T.emu_bilerp(v, ytaps=(y0 - (y0 == H - 1).long(), y1, ly)), ref, bound,
             "host.upsample2x_planes.last_row")


# ---- e. upsample + normalise ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,H,W,C", T.UPNORM_SHAPES)
def test_upsample_norm_bar(B, H, W, C):
    g = T.upnorm_input(B, H, W, C)
    lo, hi = T.upsample_norm_ref(g, T.UPNORM_SCALE)
    T.assert_f16_interval(T.emu_upsample_norm(g, T.UPNORM_SCALE), lo, hi, f"host.upsample_norm_f16[{B},{H},{W},{C}]")
    rejected("upsample_norm: the norm taken before the upsample", T.assert_f16_interval, T.emu_upsample_norm(g, T.UPNORM_SCALE, norm_first=True),
             lo, hi, "host.upsample_norm_f16.norm_first")
    gi = g[:, 1:-1, 1:-1].permute(0, 3, 1, 2)
    u = T.emu_bilerp(gi)
    one_rounding = (T.UPNORM_SCALE * (u / (u * u).sum(1, keepdim=True).sqrt())).half().permute(0, 2, 3, 1)
    rejected("upsample_norm: the first fp16 rounding dropped", T.assert_f16_interval, one_rounding, lo, hi, "host.upsample_norm_f16.one_rounding")
