"""Op-level fp64 tests of the output tail -- the kernels every inference forward ends in (csrc/elementwise.hip, csrc/corr.hip): the 2x2-cell
gram (pixel_gram_kernel, and corr_planes' own), the per-pixel norm plane, the scaled x2 / one-pass x4 upsample of the label planes,
output_conv's x2 and the strict tail's upsample + normalise -- through their lseg_op_* entries.  References, counted bounds and fp16
intervals live in tests/tail_helpers.py, where tests/test_output_tail_host.py shows wrong variants failing the same comparisons.
Outputs live between guard words in NaN-filled buffers: nothing outside may be written, everything inside must be."""
import ctypes as C

import pytest
import torch

pytestmark = [pytest.mark.gpu, pytest.mark.gpu_fast]

from lseg_hip import _lib  # noqa: E402
import tail_helpers as T  # noqa: E402

FP = torch.float16
ERR_INVALID, ERR_UNSUPPORTED = -1, -5


@pytest.fixture(scope="module")
def lib():
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    return _lib.load()


def P(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


_KEEP = []


def dev(t):
    """Upload an input and keep the device copy alive until the test ends (a temporary's memory may be handed out again at once)."""
    d = t.cuda()
    _KEEP.append(d)
    return P(d)


@pytest.fixture(autouse=True)
def _release_inputs():
    yield
    torch.cuda.synchronize()
    _KEEP.clear()


def st():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def sync():
    torch.cuda.synchronize()


# ---- a. the 2x2-cell gram --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,H,W,Cc", T.GRAM_SHAPES)
def test_pixel_gram(lib, B, H, W, Cc):
    """NV = 1 / 2 (C <= 512 / above), lanes beyond C, W % 4 in {0, 1, 2, 3} with the clamped fifth column, one run per row.  The padded
    border holds random finite values and takes part in the last row's and column's records.  At C = 512 corr_planes' gram of the
    same g -- an independent producer of the same records -- is held to the same bound."""
    g = T.feature_map(B, H, W, Cc, 10 + Cc, None, FP)
    ref, mag = T.gram_ref(g)
    bound = T.gram_bound(mag, Cc)
    out = T.Guarded((B, H, W, 5), torch.float32)
    _lib.check(lib.lseg_op_pixel_gram(dev(g), P(out.t), B, H, W, Cc, st()))
    sync()
    out.check("pixel_gram")
    T.assert_within(out.t, ref, bound, f"pixel_gram[{B},{H},{W},{Cc}]")
    if Cc == 512:
        K = 5
        t16 = T.randn((K, Cc), 11, Cc ** -0.5, FP)
        planes = torch.full((B, K, (H + 2) * (W + 2)), float("nan"), device="cuda")
        out2 = T.Guarded((B, H, W, 5), torch.float32)
        _lib.check(lib.lseg_op_corr_planes(dev(g), dev(t16), P(planes), P(out2.t), B, K, H, W, Cc, st()))
        sync()
        out2.check("corr_planes.gram")
        T.assert_within(out2.t, ref, bound, f"corr_planes.gram[{B},{H},{W},{Cc}]")


# ---- b. the norm plane ----------------------------------------------------------------------------------------------------------------------------
def _norm_plane(lib, gram32, B, H, W, flag):
    out = T.Guarded((B, 2 * H, 2 * W), torch.float32)
    _lib.check(lib.lseg_op_norm_scale_plane(dev(gram32), P(out.t), B, H, W, T.LOGIT_SCALE, P(flag), st()))
    sync()
    return out


def _flag():
    return torch.tensor([-7, 0, -7], dtype=torch.int32).cuda()


def _flag_value(f):
    f = f.cpu()
    assert f[0] == -7 and f[2] == -7, "norm_scale_plane: wrote beside its flag"
    return f[1].item()


@pytest.mark.parametrize("rough", [0.1, None], ids=["smooth", "rough"])
@pytest.mark.parametrize("B,H,W", T.NORM_SHAPES)
def test_norm_scale_plane(lib, B, H, W, rough):
    """In isolation: the gram is the fp64 gram of a random fp16 g rounded once to fp32, the reference s / ||bilinear_fp64(g)||.  Smooth g
    (neighbours share a direction) and rough g (independent neighbours: all six cross terms matter) meet the same counted bound."""
    g = T.feature_map(B, H, W, 64, 20 + H, rough, FP)
    gram32, ref, bound, _, _ = T.norm_plane_ref(g, T.LOGIT_SCALE)
    flag = _flag()
    out = _norm_plane(lib, gram32, B, H, W, flag[1:])
    out.check("norm_scale_plane")
    T.assert_within(out.t, ref, bound, f"norm_scale_plane.{'smooth' if rough else 'rough'}[{B},{H},{W}]")
    assert _flag_value(flag) == 0, "norm_scale_plane: the flag was raised on a finite gram"
    nof = _norm_plane(lib, gram32, B, H, W, None)                          # d_flag NULL
    nof.check("norm_scale_plane.noflag")
    T.assert_bits_equal(nof.t.cpu(), out.t.cpu(), "norm_scale_plane.noflag")


@pytest.mark.parametrize("B,H,W,b,y,x", [(2, 3, 7, 1, 1, 2), (1, 8, 5, 0, 7, 4), (1, 2, 2, 0, 0, 0)])
def test_norm_scale_plane_flag(lib, B, H, W, b, y, x):
    """inf in the first entry of one record: the flag becomes 1 and only the output pixels that address the record (weight 0 included:
    inf * 0) leave the clean run's bits, to 0 (s * rsqrtf(inf)) or NaN.  A NaN record: the flag becomes 1."""
    g = T.feature_map(B, H, W, 64, 20 + H, None, FP)
    gram32 = T.norm_plane_ref(g, T.LOGIT_SCALE)[0]
    clean = _norm_plane(lib, gram32, B, H, W, None).t.cpu()
    bad = gram32.clone()
    bad[b, y, x, 0] = float("inf")
    flag = _flag()
    out = _norm_plane(lib, bad, B, H, W, flag[1:])
    out.check("norm_scale_plane.inf", written=False)
    assert _flag_value(flag) == 1, "norm_scale_plane: inf in the gram did not raise the flag"
    got = out.t.cpu()
    inside = torch.zeros((B, 2 * H, 2 * W), dtype=torch.bool)
    inside[b] = T.footprint(H, W, y, x)
    T.assert_bits_equal(got[~inside], clean[~inside], "norm_scale_plane.inf.outside_the_footprint")
    assert (torch.isnan(got[inside]) | (got[inside] == 0)).all() and inside.sum().item() > 0
    bad = gram32.clone()
    bad[b, y, x] = float("nan")
    flag = _flag()
    _norm_plane(lib, bad, B, H, W, flag[1:])
    assert _flag_value(flag) == 1, "norm_scale_plane: a NaN record did not raise the flag"


# ---- c. the scaled x2 and the one-pass x4 ---------------------------------------------------------------------------------------------------------
def _x4(lib, Rpad, scale, B, K, H, W, two_stage):
    low = T.Guarded((B * K, 2 * H, 2 * W), torch.float32) if two_stage else None
    out = T.Guarded((B * K, 4 * H, 4 * W), torch.float32)
    _lib.check(lib.lseg_op_upsample4x_planes_scaled(P(Rpad), P(scale), P(out.t), B, K, H, W, two_stage, P(low.t) if low else None, st()))
    sync()
    out.check("upsample4x_planes_scaled")
    if low:
        low.check("upsample2x_planes_scaled")
    return low, out


@pytest.mark.parametrize("B,K,H,W", T.X4_SHAPES)
def test_upsample4x_planes_scaled(lib, B, K, H, W):
    """2H of 4, 14, 16, 18, 34, 24, 6, 66 low rows: a single short band of UPS4_LB = 16, exactly one, a two-row last band, several;
    W = 2: 128 sub-groups with empty shares, W = 130: one sub-group with idle threads, W = 258: the x4 += 256 loop; K > 1 with B > 1:
    pl / K selects the image's scale plane.  R is padded [B*K, H+2, W+2] with a NaN border that must never be read."""
    R, scale = T.x4_inputs(B, K, H, W)
    Rpad, sc = T.pad_nan(R).cuda(), scale.cuda()
    low, two = _x4(lib, Rpad, sc, B, K, H, W, 1)
    _, one = _x4(lib, Rpad, sc, B, K, H, W, 0)
    T.check_x4_tail(low.t, two.t, one.t, R, scale, K, f"{B},{K},{H},{W}")


def test_upsample4x_planes_scaled_refusals(lib):
    """An odd W, and a W whose band does not fit the LDS (184 bytes per column against 160 KB: W = 892; 32 per column in the two-stage
    form: W = 5122), are refused before anything is launched."""
    out, low = T.Guarded((4096,), torch.float32), T.Guarded((4096,), torch.float32)
    src = torch.zeros(1 << 16, device="cuda")
    s = st()
    assert lib.lseg_op_upsample4x_planes_scaled(P(src), P(src), P(out.t), 1, 1, 2, 7, 0, None, s) == ERR_UNSUPPORTED
    assert lib.lseg_op_upsample4x_planes_scaled(P(src), P(src), P(out.t), 1, 1, 2, 7, 1, P(low.t), s) == ERR_UNSUPPORTED
    assert lib.lseg_op_upsample4x_planes_scaled(P(src), P(src), P(out.t), 1, 1, 2, 892, 0, None, s) == ERR_UNSUPPORTED
    assert b"163840" in lib.lseg_last_error(None)
    assert lib.lseg_op_upsample4x_planes_scaled(P(src), P(src), P(out.t), 1, 1, 2, 5122, 1, P(low.t), s) == ERR_UNSUPPORTED
    assert b"163840" in lib.lseg_last_error(None)
    assert lib.lseg_op_upsample4x_planes_scaled(P(src), P(src), P(out.t), 1, 1, 1, 8, 0, None, s) == ERR_INVALID
    sync()
    out.untouched("upsample4x_planes_scaled.refusals")
    low.untouched("upsample4x_planes_scaled.refusals")


# ---- d. output_conv's x2 on planes (the evaluator tests' oracle) ----------------------------------------------------------------------------------
@pytest.mark.parametrize("Pn,H,W", T.X2_SHAPES)
def test_upsample2x_planes(lib, Pn, H, W):
    v = T.randn((Pn, H, W), 50 + H)
    ref, bound = T.up2_planes_ref(v)
    out = T.Guarded((Pn, 2 * H, 2 * W), torch.float32)
    _lib.check(lib.lseg_op_upsample2x_planes(dev(v), P(out.t), Pn, H, W, st()))
    sync()
    out.check("upsample2x_planes")
    T.assert_within(out.t, ref, bound, f"upsample2x_planes[{Pn},{H},{W}]")


def test_upsample2x_planes_refuses_a_width_that_is_no_multiple_of_4(lib):
    out = T.Guarded((4096,), torch.float32)
    src = torch.zeros(4096, device="cuda")
    assert lib.lseg_op_upsample2x_planes(P(src), P(out.t), 1, 2, 6, st()) == ERR_UNSUPPORTED
    sync()
    out.untouched("upsample2x_planes.refusal")


# ---- e. upsample + normalise + the two fp16 roundings ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,H,W,Cc", T.UPNORM_SHAPES)
def test_upsample_norm_f16(lib, B, H, W, Cc):
    """The tail of strict mode and of label sets beyond the LDS limit: fp16(scale * fp16(u / ||u||)), u the x2 bilinear of fp32 padded
    NHWC g whose NaN border must never be read.  NV = 1 / 2, lanes beyond C."""
    g = T.upnorm_input(B, H, W, Cc)
    lo, hi = T.upsample_norm_ref(g, T.UPNORM_SCALE)
    out = T.Guarded((B, 2 * H, 2 * W, Cc), FP)
    _lib.check(lib.lseg_op_upsample_norm_f16(dev(g), P(out.t), B, H, W, Cc, T.UPNORM_SCALE, st()))
    sync()
    out.check("upsample_norm_f16")
    T.assert_f16_interval(out.t, lo, hi, f"upsample_norm_f16[{B},{H},{W},{Cc}]")


# ---- refusals of the new entries ------------------------------------------------------------------------------------------------------------------
def test_refusals(lib):
    o32, o16 = T.Guarded((4096,), torch.float32), T.Guarded((4096,), FP)
    i16 = torch.zeros(1 << 16, dtype=FP, device="cuda")
    i32 = torch.zeros(1 << 16, device="cuda")
    s = st()
    cases = [
        (ERR_UNSUPPORTED, lib.lseg_op_pixel_gram(P(i16), P(o32.t), 1, 2, 2, 12, s)),
        (ERR_UNSUPPORTED, lib.lseg_op_pixel_gram(P(i16), P(o32.t), 1, 2, 2, 1032, s)),
        (ERR_UNSUPPORTED, lib.lseg_op_upsample_norm_f16(P(i32), P(o16.t), 1, 2, 2, 12, 1.0, s)),
        (ERR_UNSUPPORTED, lib.lseg_op_upsample_norm_f16(P(i32), P(o16.t), 1, 2, 2, 1032, 1.0, s)),
        (ERR_INVALID, lib.lseg_op_pixel_gram(None, P(o32.t), 1, 2, 2, 8, s)),
        (ERR_INVALID, lib.lseg_op_pixel_gram(P(i16), None, 1, 2, 2, 8, s)),
        (ERR_INVALID, lib.lseg_op_pixel_gram(P(i16), P(o32.t), 0, 2, 2, 8, s)),
        (ERR_INVALID, lib.lseg_op_pixel_gram(P(i16), P(o32.t), 1, 0, 2, 8, s)),
        (ERR_INVALID, lib.lseg_op_pixel_gram(P(i16), P(o32.t), 1, 2, 0, 8, s)),
        (ERR_INVALID, lib.lseg_op_norm_scale_plane(None, P(o32.t), 1, 2, 2, 1.0, None, s)),
        (ERR_INVALID, lib.lseg_op_norm_scale_plane(P(i32), None, 1, 2, 2, 1.0, None, s)),
        (ERR_INVALID, lib.lseg_op_norm_scale_plane(P(i32), P(o32.t), 0, 2, 2, 1.0, None, s)),
        (ERR_INVALID, lib.lseg_op_norm_scale_plane(P(i32), P(o32.t), 1, 1, 2, 1.0, None, s)),
        (ERR_INVALID, lib.lseg_op_norm_scale_plane(P(i32), P(o32.t), 1, 2, 1, 1.0, None, s)),
        (ERR_INVALID, lib.lseg_op_upsample_norm_f16(None, P(o16.t), 1, 2, 2, 8, 1.0, s)),
        (ERR_INVALID, lib.lseg_op_upsample_norm_f16(P(i32), None, 1, 2, 2, 8, 1.0, s)),
        (ERR_INVALID, lib.lseg_op_upsample_norm_f16(P(i32), P(o16.t), 0, 2, 2, 8, 1.0, s)),
        (ERR_INVALID, lib.lseg_op_upsample_norm_f16(P(i32), P(o16.t), 1, 1, 2, 8, 1.0, s)),
        (ERR_INVALID, lib.lseg_op_upsample_norm_f16(P(i32), P(o16.t), 1, 2, 1, 8, 1.0, s)),
    ]
    sync()
    for k, (want, got) in enumerate(cases):
        assert got == want, f"refusal case {k}: returned {got}, expected {want}"
    o32.untouched("refusals")
    o16.untouched("refusals")
