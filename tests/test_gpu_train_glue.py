"""Op-level tests of the training backward's data-movement kernels (csrc/elementwise.hip) through their lseg_op_* entries: the ViT
embedding / readout gradients, the DPT neck's ConvTranspose and stride-2 conv backward helpers, the split-K partial sums and the
BatchNorm running statistics.  Each is a permutation, a short fixed-order fp32 sum or a rounding, so each is held to bit equality or to
a bound counted from its operations (tests/glue_helpers.py, where tests/test_train_glue_host.py shows wrong variants failing the same
comparisons) -- not to the 10-15 % bars the whole-network gradient tests need behind 24 bf16 blocks.  Outputs live between guard
words in NaN-filled buffers: nothing outside may be written, everything inside must be."""
import ctypes as C
import math

import pytest
import torch
import torch.nn.functional as F

pytestmark = [pytest.mark.gpu, pytest.mark.gpu_fast]

from lseg_hip import _lib  # noqa: E402
import glue_helpers as G  # noqa: E402

DT = {torch.float32: _lib.LSEG_F32, torch.float16: _lib.LSEG_F16, torch.bfloat16: _lib.LSEG_BF16}
BF, FP = torch.bfloat16, torch.float16
ERR_INVALID, ERR_UNSUPPORTED = -1, -5
POS_SHAPES = [(24, 30, 30, 64), (24, 24, 24, 8), (24, 6, 10, 64), (4, 7, 3, 8), (2, 2, 5, 8)]


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


# ---- pos-embed resize -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("g_old,gh,gw,D", POS_SHAPES)
def test_pos_resize(lib, g_old, gh, gw, D):
    pos = G.randn((1 + g_old * g_old, D), 100 + gh)
    out = G.Guarded((1 + gh * gw, D), torch.float32)
    _lib.check(lib.lseg_op_pos_resize(dev(pos), P(out.t), g_old, gh, gw, D, st()))
    sync()
    out.check("pos_resize")
    if (gh, gw) == (g_old, g_old):
        G.assert_bits_equal(out.t.cpu(), pos, "pos_resize.identity")
        return
    ref, bound = G.pos_resize_ref(pos, g_old, gh, gw)
    G.assert_within(out.t, ref, bound, f"pos_resize[{g_old}->{gh}x{gw}]")


@pytest.mark.parametrize("g_old,gh,gw,D", POS_SHAPES)
def test_pos_resize_backward(lib, g_old, gh, gw, D):
    dpos = G.randn((1 + gh * gw, D), 110 + gh)
    pe0, cls0 = G.randn((1 + g_old * g_old, D), 111), G.randn((D,), 112)
    ref, bound, rcls, bcls = G.pos_resize_backward_ref(dpos, pe0, cls0, g_old, gh, gw)
    d = dpos.cuda()
    runs = []
    for _ in range(2):                                       # += into non-zero destinations, twice on the same input: bit-equal
        pe, cl = G.Guarded(pe0.shape, torch.float32, fill=pe0), G.Guarded(cls0.shape, torch.float32, fill=cls0)
        _lib.check(lib.lseg_op_pos_resize_backward(P(d), P(pe.t), P(cl.t), g_old, gh, gw, D, st()))
        sync()
        pe.check("pos_resize_backward")
        cl.check("pos_resize_backward.cls")
        runs.append((pe.t.cpu(), cl.t.cpu()))
    G.assert_bits_equal(runs[1][0], runs[0][0], "pos_resize_backward.repeat")
    G.assert_bits_equal(runs[1][1], runs[0][1], "pos_resize_backward.repeat.cls")
    G.assert_within(runs[0][0], ref, bound, f"pos_resize_backward[{g_old}->{gh}x{gw}]")
    G.assert_within(runs[0][1], rcls, bcls, f"pos_resize_backward.cls[{g_old}->{gh}x{gw}]")
    pe = G.Guarded(pe0.shape, torch.float32, fill=pe0)       # dcls NULL
    _lib.check(lib.lseg_op_pos_resize_backward(P(d), P(pe.t), None, g_old, gh, gw, D, st()))
    sync()
    pe.check("pos_resize_backward.nocls")
    G.assert_bits_equal(pe.t.cpu(), runs[0][0], "pos_resize_backward.nocls")


@pytest.mark.parametrize("g_old,gh,gw,D", [(24, 30, 30, 64), (24, 6, 10, 64)])
def test_pos_resize_adjoint(lib, g_old, gh, gw, D):
    """<resize(p), q> = <p, resize^T(q)> on the kernels' own outputs: a pair that agrees with torch separately but uses different taps
    at a clamp fails here.  Inner products in fp64; fp32 outputs carry ~1e-7 relative error each, the bar is 1e-5."""
    p, q = G.randn((1 + g_old * g_old, D), 120), G.randn((1 + gh * gw, D), 121)
    fwd = torch.full((1 + gh * gw, D), float("nan"), device="cuda")
    bwd = torch.zeros((1 + g_old * g_old, D), device="cuda")
    _lib.check(lib.lseg_op_pos_resize(dev(p), P(fwd), g_old, gh, gw, D, st()))
    _lib.check(lib.lseg_op_pos_resize_backward(dev(q), P(bwd), None, g_old, gh, gw, D, st()))
    sync()
    lhs, rhs = (fwd.cpu().double() * q.double()).sum().item(), (p.double() * bwd.cpu().double()).sum().item()
    bar = 1e-5 * max(abs(lhs), abs(rhs))
    print(f"glue-ratio pos_resize_adjoint[{g_old}->{gh}x{gw}]: |lhs-rhs| / (1e-5 * max(|lhs|, |rhs|)) = {abs(lhs - rhs) / bar:.4f}")
    assert abs(lhs - rhs) <= bar


# ---- embedding / readout --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [BF, FP])
@pytest.mark.parametrize("B,ntok,D", [(1, 5, 8), (3, 37, 192), (8, 10, 64)])
def test_embed_backward(lib, B, ntok, D, dtype):
    gx = G.randn((B, ntok, D), 130 + B)
    ref_tok, ref_pos, bound = G.embed_backward_ref(gx, dtype)
    dtok, dpos = G.Guarded(ref_tok.shape, dtype), G.Guarded((ntok, D), torch.float32)
    _lib.check(lib.lseg_op_embed_backward(dev(gx), P(dtok.t), P(dpos.t), B, ntok, D, DT[dtype], st()))
    sync()
    dtok.check("embed_backward.dtok")
    dpos.check("embed_backward.dpos")
    G.assert_bits_equal(dtok.t.cpu(), ref_tok, "embed_backward.dtok")
    G.assert_within(dpos.t, ref_pos, bound, f"embed_backward.dpos[{B},{ntok},{D}]")


@pytest.mark.parametrize("dtype", [BF, FP])
@pytest.mark.parametrize("B,ntok,D", [(2, 37, 192), (1, 2, 8), (3, 65, 256)])
def test_readout_cat(lib, B, ntok, D, dtype):
    x = G.randn((B, ntok, D), 140 + B)
    ref = G.readout_cat_ref(x, dtype)
    out = G.Guarded(ref.shape, dtype)
    _lib.check(lib.lseg_op_readout_cat(dev(x), P(out.t), B, ntok, D, DT[dtype], st()))
    sync()
    out.check("readout_cat")
    G.assert_bits_equal(out.t.cpu(), ref, "readout_cat")


@pytest.mark.parametrize("dtype", [BF, FP])
@pytest.mark.parametrize("B,ntok,D", [(2, 37, 192), (1, 2, 8), (3, 65, 256), (1, 34, 264)])
def test_readout_cat_backward(lib, B, ntok, D, dtype):
    """(2, 37, 192): np = 36 is no multiple of the cls kernel's 32 row lanes and D = 192 leaves column groups of its 256-wide block idle;
    (1, 34, 264): a second, mostly idle column block (the c0 < D guard)."""
    gx0 = G.randn((B, ntok, D), 150 + B)
    dcat = G.randn((B * (ntok - 1), 2 * D), 151 + B, 0.5, dtype)
    patch, cls, bound = G.readout_cat_backward_ref(gx0, dcat)
    d, runs = dcat.cuda(), []
    for _ in range(2):
        gx = G.Guarded(gx0.shape, torch.float32, fill=gx0)
        _lib.check(lib.lseg_op_readout_cat_backward(P(d), P(gx.t), B, ntok, D, DT[dtype], st()))
        sync()
        gx.check("readout_cat_backward")
        runs.append(gx.t.cpu())
    G.assert_bits_equal(runs[1], runs[0], "readout_cat_backward.repeat")
    G.assert_bits_equal(runs[0][:, 1:].contiguous(), patch, "readout_cat_backward.patch_rows")
    G.assert_within(runs[0][:, 0], cls, bound, f"readout_cat_backward.cls[{B},{ntok},{D}]")


# ---- 16-bit map permutations --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,H,W,Cc", [(2, 5, 7, 8), (1, 15, 15, 64)])
def test_unpad_rows(lib, B, H, W, Cc):
    for dtype in (BF, FP):
        x = G.with_specials16(G.randn((B, H + 2, W + 2, Cc), 160 + H, dtype=dtype))
        out = G.Guarded((B * H * W, Cc), dtype)
        _lib.check(lib.lseg_op_unpad_rows(dev(x), P(out.t), B, H, W, Cc, st()))
        sync()
        out.check("unpad_rows")
        G.assert_bits_equal(out.t.cpu(), G.unpad_rows_ref(x), "unpad_rows")


@pytest.mark.parametrize("B,H,W,Cc", [(1, 15, 15, 8), (2, 30, 16, 64), (1, 2, 3, 8)])
def test_dilate2(lib, B, H, W, Cc):
    Ho, Wo = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    dy = G.with_specials16(G.randn((B, Ho + 2, Wo + 2, Cc), 170 + H, dtype=BF))      # its border is finite garbage: never copied
    out = G.Guarded((B, H + 2, W + 2, Cc), BF)
    _lib.check(lib.lseg_op_dilate2(dev(dy), P(out.t), B, H, W, Cc, st()))
    sync()
    out.check("dilate2")
    got, ref = out.t.cpu(), G.dilate2_ref(dy, H, W)
    G.assert_bits_equal(got, ref, "dilate2")
    even = torch.zeros((H + 2, W + 2), dtype=torch.bool)
    even[1:1 + 2 * Ho:2, 1:1 + 2 * Wo:2] = True
    assert even.sum().item() == Ho * Wo and not got.view(torch.int16)[:, ~even].any(), "dilate2: non-zero bits off the even sites"


@pytest.mark.parametrize("B,gh,gw,s,Cc", [(2, 3, 5, 4, 8), (1, 6, 4, 2, 64), (1, 1, 1, 4, 8)])
def test_unpixshuf(lib, B, gh, gw, s, Cc):
    dl = G.with_specials16(G.randn((B, gh * s + 2, gw * s + 2, Cc), 180 + gh, dtype=FP))
    out = G.Guarded((B * gh * gw, s * s * Cc), FP)
    _lib.check(lib.lseg_op_unpixshuf(dev(dl), P(out.t), B, gh, gw, s, Cc, st()))
    sync()
    out.check("unpixshuf")
    G.assert_bits_equal(out.t.cpu(), G.unpixshuf_ref(dl, gh, gw, s), "unpixshuf")


# ---- ConvTranspose2d(kernel = stride = s): packed weight, and the backward as the training step composes it --------------------------------
@pytest.mark.parametrize("B,gh,gw,Cc,Cp,s", [(1, 3, 5, 48, 64, 4), (2, 4, 4, 64, 64, 2), (1, 2, 2, 128, 128, 4)])
def test_convT_backward_composed(lib, B, gh, gw, Cc, Cp, s):
    """pack_convT, then unpixshuf -> linear_backward -> convT_wgrad_unpack + fold_rows(R = s*s, ld = Cp) against fp64 autograd of
    F.conv_transpose2d on the bf16-rounded operands.  Padded channels (Cc < Cp) of the rows and of the gradient map, and the map's
    border, hold finite garbage: none of it may reach the weight or bias gradient."""
    M = B * gh * gw
    x = G.randn((B, Cc, gh, gw), 190, dtype=BF)
    w = G.randn((Cc, Cc, s, s), 191, Cc ** -0.5, BF).float()
    b = G.randn((Cc,), 192)
    dL = G.randn((B, Cc, gh * s, gw * s), 193, 0.5, BF)
    # forward twin: the packed weight.  Only the Cc x Cc real entries are written: a non-zero pattern in the padding must survive
    # bit for bit; the zero-filled copy is the one the products below use (the caller zeroes the padding once).
    for fill in (G.randn((s * s * Cp, Cp), 198, dtype=BF), torch.zeros((s * s * Cp, Cp), dtype=BF)):
        wp = G.Guarded(fill.shape, BF, fill=fill)
        _lib.check(lib.lseg_op_pack_convT(dev(w), P(wp.t), Cc, Cc, Cp, s, DT[BF], st()))
        sync()
        wp.check("pack_convT")
        G.assert_bits_equal(wp.t.cpu(), G.pack_convT_ref(w, Cp, s, BF, fill), "pack_convT")
    rows = G.randn((M, Cp), 194, dtype=BF)
    rows[:, :Cc] = x.permute(0, 2, 3, 1).reshape(M, Cc)
    clean = rows.clone()
    clean[:, Cc:] = 0
    fwd = G.convT_forward_from_packed(clean, wp.t.cpu(), B, gh, gw, s, Cp)
    want = F.conv_transpose2d(x.double(), w.double(), None, stride=s)
    G.check_convT_forward(fwd, want, Cc, "pack_convT.forward")
    # backward
    ref_dw, ref_db = G.convT_backward_autograd(x, w, b, dL, s)
    dl = G.randn((B, gh * s + 2, gw * s + 2, Cp), 195, dtype=BF)
    dl[:, 1:-1, 1:-1, :Cc] = dL.permute(0, 2, 3, 1)
    dG = G.Guarded((M, s * s * Cp), BF)
    _lib.check(lib.lseg_op_unpixshuf(dev(dl), P(dG.t), B, gh, gw, s, Cp, st()))
    dwg = torch.full((s * s * Cp, Cp), float("nan"), device="cuda")
    dbg = torch.full((s * s * Cp,), float("nan"), device="cuda")
    _lib.check(lib.lseg_op_linear_backward(P(dG.t), dev(rows), P(wp.t), DT[BF], None, P(dwg), P(dbg), M, s * s * Cp, Cp, st()))
    pre_w, pre_b = G.randn((Cc, Cc, s, s), 196), G.randn((Cc,), 197)
    for acc in (0, 1):
        dw = G.Guarded(pre_w.shape, torch.float32, fill=pre_w if acc else None)
        db = G.Guarded(pre_b.shape, torch.float32, fill=pre_b if acc else None)
        _lib.check(lib.lseg_op_convT_wgrad_unpack(P(dwg), P(dw.t), Cc, Cp, s, acc, st()))
        _lib.check(lib.lseg_op_fold_rows(P(dbg), P(db.t), s * s, Cc, Cp, acc, st()))
        sync()
        dG.check("convT.unpixshuf")
        dw.check("convT_wgrad_unpack")
        db.check("convT.fold_rows")
        G.check_convT_grads(dw.t, db.t, ref_dw + (pre_w.double() if acc else 0), ref_db + (pre_b.double() if acc else 0),
                            f"convT_backward[{B},{gh},{gw},{Cc},{Cp},{s}].acc{acc}")
    # the unpack itself is a permutation of the GEMM's result: exact
    G.assert_bits_equal(_unpack_once(lib, dwg, Cc, Cp, s), G.convT_wgrad_unpack_ref(dwg.cpu(), Cc, Cp, s), "convT_wgrad_unpack.permutation")


def _unpack_once(lib, dwg, Cc, Cp, s):
    out = torch.full((Cc, Cc, s, s), float("nan"), device="cuda")
    _lib.check(lib.lseg_op_convT_wgrad_unpack(P(dwg), P(out), Cc, Cp, s, 0, st()))
    sync()
    return out.cpu()


@pytest.mark.parametrize("B,H,W,Cin,Cout", [(1, 15, 15, 64, 64), (2, 16, 30, 128, 64)])
def test_conv_s2_backward_composed(lib, B, H, W, Cin, Cout):
    """dilate2 -> conv3x3_backward on the dilated map -> unpad_rows against fp64 autograd of F.conv2d(stride=2, padding=1)."""
    Ho, Wo = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    x = G.randn((B, Cin, H, W), 200, dtype=BF)
    w = G.randn((Cout, Cin, 3, 3), 201, 1 / math.sqrt(9 * Cin), BF)
    dy = G.randn((B, Cout, Ho, Wo), 202, dtype=BF)
    ref_dx, ref_dw = G.conv_s2_backward_autograd(x, w, dy)
    xp = torch.zeros((B, H + 2, W + 2, Cin), dtype=BF)
    xp[:, 1:-1, 1:-1] = x.permute(0, 2, 3, 1)
    dyp = G.randn((B, Ho + 2, Wo + 2, Cout), 203, dtype=BF)                            # border: finite garbage dilate2 must not copy
    dyp[:, 1:-1, 1:-1] = dy.permute(0, 2, 3, 1)
    wpk = w.permute(0, 2, 3, 1).reshape(Cout, 9 * Cin).contiguous()
    dyd = G.Guarded((B, H + 2, W + 2, Cout), BF)
    dxp = torch.zeros((B, H + 2, W + 2, Cin), dtype=BF, device="cuda")
    dw = torch.full((Cout, 9 * Cin), float("nan"), device="cuda")
    rows = G.Guarded((B * H * W, Cin), BF)
    _lib.check(lib.lseg_op_dilate2(dev(dyp), P(dyd.t), B, H, W, Cout, st()))
    _lib.check(lib.lseg_op_conv3x3_backward(P(dyd.t), dev(xp), dev(wpk), P(dxp), P(dw), B, H, W, Cin, Cout, st()))
    _lib.check(lib.lseg_op_unpad_rows(P(dxp), P(rows.t), B, H, W, Cin, st()))
    sync()
    dyd.check("conv_s2.dilate2")
    rows.check("conv_s2.unpad_rows")
    got_dx = rows.t.cpu().float().reshape(B, H, W, Cin).permute(0, 3, 1, 2)
    got_dw = dw.cpu().reshape(Cout, 3, 3, Cin).permute(0, 3, 1, 2)
    G.check_conv_s2_grads(got_dx, got_dw, ref_dx, ref_dw, f"conv_s2_backward[{B},{H},{W},{Cin},{Cout}]")


# ---- fp32 partial sums ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("acc", [0, 1])
@pytest.mark.parametrize("Co,Ci,Cip,ns", [(5, 3, 8, 1), (64, 48, 64, 3), (8, 8, 8, 8)])
def test_conv_wgrad_unpack(lib, Co, Ci, Cip, ns, acc):
    Cop = Co + 3                                               # padded output rows and input columns hold garbage; so does the gap
    slab = Cop * 9 * Cip
    stride = slab + 16                                         # split_stride larger than the slab
    buf = G.randn((ns, stride), 210 + ns)
    slabs = buf[:, :slab].reshape(ns, Cop, 9, Cip)
    pre = G.randn((Co, Ci, 3, 3), 211) if acc else None
    ref, bound, terms = G.conv_wgrad_unpack_ref(slabs, Co, Ci, pre)
    out = G.Guarded((Co, Ci, 3, 3), torch.float32, fill=pre)
    _lib.check(lib.lseg_op_conv_wgrad_unpack(dev(buf), P(out.t), Co, Ci, Cip, acc, ns, stride, st()))
    sync()
    out.check("conv_wgrad_unpack")
    if terms == 1:
        G.assert_bits_equal(out.t.cpu(), ref.float(), "conv_wgrad_unpack.single")
    else:
        G.assert_within(out.t, ref, bound, f"conv_wgrad_unpack[{Co},{Ci},{Cip},{ns},acc{acc}]")


@pytest.mark.parametrize("acc", [0, 1])
@pytest.mark.parametrize("ns,n", [(1, 4), (5, 4 * 1031), (8, 4096)])
def test_sum_partials(lib, ns, n, acc):
    stride = n + 8                                             # stride > n
    part = G.randn((ns, stride), 220 + ns)
    pre = G.randn((n,), 221) if acc else None
    ref, bound, terms = G.sum_partials_ref(part, n, pre)
    out = G.Guarded((n,), torch.float32, fill=pre)
    _lib.check(lib.lseg_op_sum_partials(dev(part), P(out.t), ns, n, stride, acc, st()))
    sync()
    out.check("sum_partials")
    if terms == 1:
        G.assert_bits_equal(out.t.cpu(), ref.float(), "sum_partials.single")
    else:
        G.assert_within(out.t, ref, bound, f"sum_partials[{ns},{n},acc{acc}]")


@pytest.mark.parametrize("acc", [0, 1])
@pytest.mark.parametrize("R,Cc,ld", [(1, 64, 64), (16, 48, 64), (4, 300, 320)])
def test_fold_rows(lib, R, Cc, ld, acc):
    src = G.randn((R, ld), 230 + R)
    pre = G.randn((Cc,), 231) if acc else None
    ref, bound, terms = G.fold_rows_ref(src, Cc, pre)
    out = G.Guarded((Cc,), torch.float32, fill=pre)
    _lib.check(lib.lseg_op_fold_rows(dev(src), P(out.t), R, Cc, ld, acc, st()))
    sync()
    out.check("fold_rows")
    if terms == 1:
        G.assert_bits_equal(out.t.cpu(), ref.float(), "fold_rows.single")
    else:
        G.assert_within(out.t, ref, bound, f"fold_rows[{R},{Cc},{ld},acc{acc}]")


# ---- BatchNorm running statistics ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("Cc,count", [(8, 2), (64, 450), (300, 7200), (8, 1)])
def test_bn_running_update(lib, Cc, count):
    """count == 1: torch has no unbiased variance there; launch_bn_running_update documents the biased one (which is 0), so the
    running variance decays by 1 - momentum."""
    x = G.randn((count, Cc), 240 + Cc, 0.5, torch.float64) + 1.5
    rm0, rv0 = G.randn((Cc,), 241), G.randn((Cc,), 242).abs() + 0.5
    stats, rm, bm, rv, bv = G.bn_running_ref(x, rm0, rv0)
    gm, gv = G.Guarded((Cc,), torch.float32, fill=rm0), G.Guarded((Cc,), torch.float32, fill=rv0)
    _lib.check(lib.lseg_op_bn_running_update(dev(stats), P(gm.t), P(gv.t), Cc, float(count), 0.1, st()))
    sync()
    gm.check("bn_running_update.mean")
    gv.check("bn_running_update.var")
    G.assert_within(gm.t, rm, bm, f"bn_running_update.mean[{Cc},{count}]")
    G.assert_within(gv.t, rv, bv, f"bn_running_update.var[{Cc},{count}]")


# ---- refusals -------------------------------------------------------------------------------------------------------------------------------
def test_refusals(lib):
    """Each wrapper returns LSEG_ERR_INVALID / LSEG_ERR_UNSUPPORTED as the header states and launches nothing: the sentinel-filled
    outputs keep every bit."""
    o16, o32, o32b = G.Guarded((4096,), BF), G.Guarded((4096,), torch.float32), G.Guarded((64,), torch.float32)
    i16 = torch.zeros(4096, dtype=BF, device="cuda")
    i32 = torch.zeros(4096, device="cuda")
    s = st()
    bf = DT[BF]
    cases = [
        # channel counts the 16-byte lanes cannot cover (C = 12, D = 12)
        (ERR_UNSUPPORTED, lib.lseg_op_unpad_rows(P(i16), P(o16.t), 1, 2, 2, 12, s)),
        (ERR_UNSUPPORTED, lib.lseg_op_dilate2(P(i16), P(o16.t), 1, 3, 3, 12, s)),
        (ERR_UNSUPPORTED, lib.lseg_op_unpixshuf(P(i16), P(o16.t), 1, 2, 2, 2, 12, s)),
        (ERR_UNSUPPORTED, lib.lseg_op_readout_cat(P(i32), P(o16.t), 1, 3, 12, bf, s)),
        (ERR_UNSUPPORTED, lib.lseg_op_readout_cat_backward(P(i16), P(o32.t), 1, 3, 12, bf, s)),
        # n / stride no multiple of 4
        (ERR_INVALID, lib.lseg_op_sum_partials(P(i32), P(o32.t), 2, 6, 8, 0, s)),
        (ERR_INVALID, lib.lseg_op_sum_partials(P(i32), P(o32.t), 2, 8, 10, 0, s)),
        # NULL pointers
        (ERR_INVALID, lib.lseg_op_pos_resize(None, P(o32.t), 2, 2, 2, 8, s)),
        (ERR_INVALID, lib.lseg_op_pos_resize(P(i32), None, 2, 2, 2, 8, s)),
        (ERR_INVALID, lib.lseg_op_pos_resize_backward(None, P(o32.t), P(o32b.t), 2, 2, 2, 8, s)),
        (ERR_INVALID, lib.lseg_op_pos_resize_backward(P(i32), None, P(o32b.t), 2, 2, 2, 8, s)),
        (ERR_INVALID, lib.lseg_op_embed_backward(None, P(o16.t), P(o32.t), 1, 3, 8, bf, s)),
        (ERR_INVALID, lib.lseg_op_embed_backward(P(i32), None, P(o32.t), 1, 3, 8, bf, s)),
        (ERR_INVALID, lib.lseg_op_embed_backward(P(i32), P(o16.t), None, 1, 3, 8, bf, s)),
        (ERR_INVALID, lib.lseg_op_readout_cat(None, P(o16.t), 1, 3, 8, bf, s)),
        (ERR_INVALID, lib.lseg_op_readout_cat_backward(None, P(o32.t), 1, 3, 8, bf, s)),
        (ERR_INVALID, lib.lseg_op_unpad_rows(None, P(o16.t), 1, 2, 2, 8, s)),
        (ERR_INVALID, lib.lseg_op_dilate2(None, P(o16.t), 1, 3, 3, 8, s)),
        (ERR_INVALID, lib.lseg_op_unpixshuf(None, P(o16.t), 1, 2, 2, 2, 8, s)),
        (ERR_INVALID, lib.lseg_op_pack_convT(None, P(o16.t), 8, 8, 8, 2, bf, s)),
        (ERR_INVALID, lib.lseg_op_convT_wgrad_unpack(None, P(o32.t), 8, 8, 2, 0, s)),
        (ERR_INVALID, lib.lseg_op_conv_wgrad_unpack(None, P(o32.t), 8, 8, 8, 0, 1, 0, s)),
        (ERR_INVALID, lib.lseg_op_fold_rows(None, P(o32.t), 2, 8, 8, 0, s)),
        (ERR_INVALID, lib.lseg_op_sum_partials(None, P(o32.t), 2, 8, 8, 0, s)),
        (ERR_INVALID, lib.lseg_op_bn_running_update(None, P(o32.t), P(o32b.t), 8, 4.0, 0.1, s)),
        # sizes below 1, and layouts the kernel would read or write out of bounds
        (ERR_INVALID, lib.lseg_op_pos_resize(P(i32), P(o32.t), 2, 0, 2, 8, s)),
        (ERR_INVALID, lib.lseg_op_pos_resize_backward(P(i32), P(o32.t), None, 2, 2, 2, 0, s)),
        (ERR_INVALID, lib.lseg_op_embed_backward(P(i32), P(o16.t), P(o32.t), 0, 3, 8, bf, s)),
        (ERR_INVALID, lib.lseg_op_embed_backward(P(i32), P(o16.t), P(o32.t), 1, 3, 8, DT[torch.float32], s)),
        (ERR_INVALID, lib.lseg_op_readout_cat(P(i32), P(o16.t), 1, 1, 8, bf, s)),
        (ERR_INVALID, lib.lseg_op_unpad_rows(P(i16), P(o16.t), 1, 0, 2, 8, s)),
        (ERR_INVALID, lib.lseg_op_dilate2(P(i16), P(o16.t), 0, 3, 3, 8, s)),
        (ERR_INVALID, lib.lseg_op_unpixshuf(P(i16), P(o16.t), 1, 2, 2, 0, 8, s)),
        (ERR_INVALID, lib.lseg_op_pack_convT(P(i32), P(o16.t), 16, 8, 8, 2, bf, s)),
        (ERR_INVALID, lib.lseg_op_convT_wgrad_unpack(P(i32), P(o32.t), 16, 8, 2, 0, s)),
        (ERR_INVALID, lib.lseg_op_conv_wgrad_unpack(P(i32), P(o32.t), 2, 16, 8, 0, 1, 0, s)),
        (ERR_INVALID, lib.lseg_op_conv_wgrad_unpack(P(i32), P(o32.t), 2, 8, 8, 0, 2, 8, s)),
        (ERR_INVALID, lib.lseg_op_fold_rows(P(i32), P(o32.t), 2, 16, 8, 0, s)),
        (ERR_INVALID, lib.lseg_op_sum_partials(P(i32), P(o32.t), 0, 8, 8, 0, s)),
        (ERR_INVALID, lib.lseg_op_bn_running_update(P(i32), P(o32.t), P(o32b.t), 8, 0.0, 0.1, s)),
    ]
    sync()
    for k, (want, got) in enumerate(cases):
        assert got == want, f"refusal case {k}: returned {got}, expected {want}"
    for g in (o16, o32, o32b):
        g.untouched("refusals")
