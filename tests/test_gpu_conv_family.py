"""Op-level fp64 tests of the conv family: the CONV instantiations of the GEMM kernel through lseg_op_conv_ex (3x3 and 1x1, stride 1 and 2,
64x64 / 128x128 / 256x256 tiles, the generic and the padded-NHWC epilogue with ReLU, relu_in, one and two skips, relu_after_res, the ReLU
copy, the in-place skip; split-K slabs), conv_reduce_pad, the split launch + reduction end to end, the K-major conv and linear weight
gradients and the weight packers, in bf16 and fp16.  Every forward case first asserts, through lseg_op_conv_ex_plan at this device's CU
count, that it runs the epilogue, the tile and the work items per workgroup it was written for.  References, counted bounds, intervals,
guarded buffers: tests/conv_helpers.py; tests/test_conv_family_host.py shows wrong variants failing the same comparisons."""
import ctypes as C

import pytest
import torch

pytestmark = [pytest.mark.gpu, pytest.mark.gpu_fast]

from lseg_hip import _lib  # noqa: E402
import conv_helpers as H  # noqa: E402
import gemm_helpers as G  # noqa: E402

ERR_INVALID, ERR_UNSUPPORTED = -1, -5


@pytest.fixture(scope="module")
def lib():
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    return _lib.load()


@pytest.fixture(scope="module")
def cus():
    return torch.cuda.get_device_properties(0).multi_processor_count


def stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def launch_conv(lib, cus, c, d, outs, expect=0, **over):
    dev = {k: d[k].cuda() for k in ("x", "W", "bias", "res", "res2")}
    ptrs = {k: t.data_ptr() for k, t in dev.items()}
    ptrs["out"] = outs["out"].ptr()
    ptrs["out_relu"] = outs["out_relu"].ptr() if "out_relu" in outs else 0
    g = H.struct_of(c, ptrs)
    for k, v in over.items():
        setattr(g, k, v)
    if expect == 0:
        H.assert_plan(lib, c, g, cus)
    r = lib.lseg_op_conv_ex(C.byref(g), stream())
    torch.cuda.synchronize()
    assert r == expect, f"{c['name']}: lseg_op_conv_ex returned {r}, expected {expect}: {lib.lseg_last_error(None)}"
    return outs


@pytest.mark.parametrize("c", H.GEOMETRY, ids=H.ids(H.GEOMETRY))
def test_forward_geometry_and_tiles(lib, cus, c):
    """a. Cin 64 | 128 x Cout 64 (generic, 64x64) | 128 (PAD16, 64x64 and 128x128) | 256 (PAD16, 256x256); stride-1 maps with M = 105, 144, 300
    (ragged last tile, tile rows straddling images), stride-2 maps 7x5 and 6x8 at 3x3 and at 1x1; max_grid = 8 walks of 2 .. 3 tiles.
    The input border is random and non-zero, the output border is guard pattern."""
    d = H.fdata(c)
    H.check_forward(c, d, launch_conv(lib, cus, c, d, H.make_fouts(c, d, "cuda")))


@pytest.mark.parametrize("c", H.EPILOGUE, ids=H.ids(H.EPILOGUE))
def test_forward_epilogue_forms(lib, cus, c):
    """b. no ReLU / ReLU, relu_in (bf16 AND fp16), res, res + res2, relu_after_res with one and two skips, out_relu with and without skips
    (bit for bit the stored out with its negative halves cleared), out aliasing res."""
    d = H.fdata(c)
    H.check_forward(c, d, launch_conv(lib, cus, c, d, H.make_fouts(c, d, "cuda")))


def test_out_relu_off_the_specialised_epilogue_is_refused(lib, cus):
    c = dict(next(x for x in H.EPILOGUE if x["name"] == "epi.plain.co64.t1.bf16"), out_relu=1)
    d = H.fdata(c)
    outs = launch_conv(lib, cus, c, d, H.make_fouts(c, d, "cuda"), expect=ERR_UNSUPPORTED)
    outs["out"].untouched(c["name"])
    outs["out_relu"].untouched(c["name"])


@pytest.mark.parametrize("c", H.SPLIT, ids=H.ids(H.SPLIT))
def test_split_k_conv_slabs(lib, cus, c):
    """c. PART32 with CONV at Cin = 128 on tiles 1, 2, 6: 4 x 5 of 18 steps (odd: ranges begin mid-tap; short last range), 6 x 3, 18 x 1,
    2 x 9.  Each slab against the fp64 partial sum of exactly its K-range; the slab behind the last one keeps its pattern."""
    d = H.fdata(c)
    H.check_split(c, d, launch_conv(lib, cus, c, d, H.make_souts(c, d, "cuda")))


def run_reduce(lib, c, d, part, outs, ns=None, stride=None):
    dev = {k: d[k].cuda() for k in ("bias", "res", "res2")}
    M = c["B"] * c["Ho"] * c["Wo"]
    res = (outs["out"].ptr() if c["alias"] else dev["res"].data_ptr()) if c["nres"] >= 1 else None
    r = lib.lseg_op_conv_reduce_pad(part.data_ptr(), ns or c["ns"], stride or (M + 1) * c["C"], dev["bias"].data_ptr() if c["bias"] else None, res,
                                    dev["res2"].data_ptr() if c["nres"] >= 2 else None, outs["out"].ptr(),
                                    outs["out_relu"].ptr() if c["out_relu"] else None, c["B"], c["Ho"], c["Wo"], c["C"], c["relu"], c["rar"],
                                    G.LD[c["dt"]], stream())
    torch.cuda.synchronize()
    assert r == 0, f"{c['name']}: {r}: {lib.lseg_last_error(None)}"
    return outs


@pytest.mark.parametrize("c", H.REDUCE, ids=H.ids(H.REDUCE))
def test_conv_reduce_pad(lib, c):
    """c. ns in {2, 3, 8} x C in {8, 64, 256} with every epilogue form the reduction implements, slabs a row of slack apart."""
    d = H.rdata(c)
    H.check_reduce(c, d, run_reduce(lib, c, d, d["part"].cuda(), H.make_routs(c, d, "cuda")))


@pytest.mark.parametrize("dt", ["bf16", "f16"])
def test_split_launch_plus_reduction_against_the_unsplit_conv(lib, cus, dt):
    """c. end to end, Engine::conv3x3's small-batch path: split launch (4 x 5 of 18 steps) + conv_reduce_pad with bias, ReLU, two skips and
    the ReLU copy, against the fp64 reference within the sum of the slab and the reduction bounds, and against the unsplit
    lseg_op_conv_ex of the same problem within the width of the interval both bounds give together."""
    sc = next(x for x in H.SPLIT if x["name"] == f"split.t2.4x5.{dt}")
    d = H.fdata(sc)
    slabs = launch_conv(lib, cus, sc, d, H.make_souts(sc, d, "cuda"))["out"]
    B, (Ho, Wo), N, ns = sc["B"], H.out_hw(sc), sc["Cout"], sc["nsplit"]
    fc = dict(sc, name=f"e2e.unsplit.{dt}", nsplit=0, steps=0, relu=1, nres=2, out_relu=1, max_grid=0, exp=(H.EPI_PAD16, 2, 1))
    un = launch_conv(lib, cus, fc, d, H.make_fouts(fc, d, "cuda"))
    H.check_forward(fc, d, un)
    rc = dict(name=f"e2e.reduce.{dt}", B=B, Ho=Ho, Wo=Wo, C=N, ns=ns, dt=dt, relu=1, nres=2, rar=0, out_relu=1, alias=0, bias=1)
    outs = H.make_routs(rc, d, "cuda")
    run_reduce(lib, rc, d, slabs.payload(), outs, stride=B * Ho * Wo * N)
    rd = dict(d, part=slabs.payload()[:ns].cpu().reshape(ns, B * Ho * Wo, N))
    rd["part"] = torch.cat([rd["part"], torch.zeros(ns, 1, N)], 1)                 # rinterval's row of slack
    H.check_reduce(rc, rd, outs)                                                   # the reduction of THESE slabs, within its own bound
    lo1, hi1 = H.finterval(fc, d)                                                  # the unsplit conv's interval: bound over the whole K
    lo2, hi2 = H.rinterval(rc, rd)
    _, must, _, b = H.split_ref(sc, d)
    slab_b = b[:ns].sum(0).reshape(B, Ho, Wo, N)                                   # what the slabs themselves may be off by
    got_s, got_u = outs["out"].payload().cpu()[:, 1:-1, 1:-1].double(), un["out"].payload().cpu()[:, 1:-1, 1:-1].double()
    lo = G.round_to(torch.minimum(lo1, lo2 - slab_b), dt).reshape(got_s.shape)
    hi = G.round_to(torch.maximum(hi1, hi2 + slab_b), dt).reshape(got_s.shape)
    assert ((got_s >= lo) & (got_s <= hi) & (got_u >= lo) & (got_u <= hi)).all(), "split + reduce and the unsplit conv differ by more than both bounds"
    print(f"conv-ratio e2e.{dt}: split + reduce == unsplit bit for bit on {100 * (got_s == got_u).double().mean().item():.2f} % of the outputs")


@pytest.mark.parametrize("c", H.WGRAD, ids=H.ids(H.WGRAD))
def test_conv_wgrad_kmajor(lib, c):
    """d. Cin 128 | 256 (one | two column tiles per tap), Cout 64 | 192 (below the 128-row tile | ragged); B = 1 6x5: one K-step with a
    k_valid tail, shifted rows below 0 and above k_valid; B = 2 22x22: 2 slabs, and 1 slab with a workspace of exactly one; relu_x 0 | 1.
    Both maps lie between rows of a finite non-zero poison, so a row read outside [0, k_valid) shows whatever the allocator holds."""
    d = H.wdata(c)
    out = H.wgrad_out(c, "cuda")
    n = H.wgrad_ws_floats(c)
    ws = torch.full((n + 64,), 7.0, device="cuda")
    (xbuf, x), (dybuf, dy) = H.poisoned(d["x"], "cuda"), H.poisoned(d["dy"], "cuda")      # finite non-zero rows before and behind both maps
    ns = lib.lseg_op_conv_wgrad(dy.data_ptr(), x.data_ptr(), out.ptr(), c["relu_x"], c["B"], c["H"], c["W"], c["Cin"], c["Cout"], ws.data_ptr(), n,
                                G.LD[c["dt"]], stream())
    torch.cuda.synchronize()
    assert ns >= 1, f"{c['name']}: {ns}: {lib.lseg_last_error(None)}"
    assert (ws[n:] == 7.0).all(), f"{c['name']}: the launch wrote behind its workspace"
    H.check_wgrad(c, d, out, ns)


@pytest.mark.parametrize("c", H.WLIN, ids=H.ids(H.WLIN))
def test_linear_wgrad_kmajor(lib, c):
    """d. M in {37, 64, 130} (tail | exact | two K-steps and a tail), rows_out = 40 < ldy = 48, cols_out 128 | 384 < ldx, accumulate 0 | 1."""
    d = H.ldata(c)
    out = H.wlin_out(c, d, "cuda")
    n = c["rows"] * c["cols"]
    ws = torch.full((n + 64,), 7.0, device="cuda")
    (xbuf, x), (dybuf, dy) = H.poisoned(d["x"], "cuda"), H.poisoned(d["dy"], "cuda")      # rows M .. of the last K-step are poison, not zeros
    r = lib.lseg_op_wgrad_kmajor(dy.data_ptr(), c["ldy"], x.data_ptr(), c["ldx"], c["M"], c["rows"], c["cols"], out.ptr(), c["acc"], ws.data_ptr(), n,
                                 G.LD[c["dt"]], stream())
    torch.cuda.synchronize()
    assert r == 0, f"{c['name']}: {r}: {lib.lseg_last_error(None)}"
    assert (ws[n:] == 7.0).all(), f"{c['name']}: the launch wrote behind its workspace"
    H.check_wlin(c, d, out)


def test_wgrad_refusals_launch_nothing(lib):
    """Cin % 128 != 0, cols_out % 128 != 0, workspace too small: refused by return code, output and workspace untouched."""
    c = H.WGRAD[0]
    d = H.wdata(c)
    out = H.wgrad_out(c, "cuda")
    ws = torch.full((c["Cout"] * 9 * c["Cin"],), 7.0, device="cuda")
    x, dy = d["x"].cuda(), d["dy"].cuda()
    args = lambda Cin, n: (dy.data_ptr(), x.data_ptr(), out.ptr(), 0, c["B"], c["H"], c["W"], Cin, c["Cout"], ws.data_ptr(), n, G.LD[c["dt"]], stream())
    assert lib.lseg_op_conv_wgrad(*args(64, ws.numel())) == ERR_UNSUPPORTED
    assert lib.lseg_op_conv_wgrad(*args(c["Cin"], ws.numel() - 4)) == ERR_UNSUPPORTED
    lc = H.WLIN[0]
    ld = H.ldata(lc)
    lout = H.wlin_out(lc, ld, "cuda")
    lx, ldy = ld["x"].cuda(), ld["dy"].cuda()
    la = lambda cols, n: (ldy.data_ptr(), lc["ldy"], lx.data_ptr(), lc["ldx"], lc["M"], lc["rows"], cols, lout.ptr(), 0, ws.data_ptr(), n, G.LD[lc["dt"]], stream())
    assert lib.lseg_op_wgrad_kmajor(*la(64, ws.numel())) == ERR_UNSUPPORTED
    assert lib.lseg_op_wgrad_kmajor(*la(lc["cols"], lc["rows"] * lc["cols"] - 4)) == ERR_UNSUPPORTED
    torch.cuda.synchronize()
    out.untouched(c["name"])
    lout.untouched(lc["name"])
    assert (ws == 7.0).all()


@pytest.mark.parametrize("c", H.DGRAD_PACK, ids=H.ids(H.DGRAD_PACK))
def test_conv_dgrad_pack_is_the_flipped_transposed_weight(lib, c):
    d = H.dgrad_pack_data(c)
    shape = (c["Ci"], 9, c["Co"])
    out = G.Out(shape, c["dt"], torch.ones(shape, dtype=torch.bool), "cuda")
    wp = d["wp"].cuda()
    assert lib.lseg_op_conv_dgrad_pack(wp.data_ptr(), out.ptr(), c["Co"], c["Ci"], stream()) == 0, lib.lseg_last_error(None)
    torch.cuda.synchronize()
    G.assert_bits_equal(out.check(c["name"]), H.dgrad_pack_ref(d).reshape(shape), c["name"])


@pytest.mark.parametrize("c", H.PACK3 + H.PACK1, ids=H.ids(H.PACK3 + H.PACK1))
def test_folding_packers(lib, c):
    """e. pack_conv3x3 with / without BatchNorm and conv bias, Ci = 3 -> Cip = 64 and Ci = Cip, fp32 / bf16 / fp16 output; pack_conv1x1 with
    and without BatchNorm.  The pad channels hold the caller's zeros and keep them."""
    d = H.pdata(c)
    dev = {k: v.cuda() for k, v in d.items()}
    outs = H.make_pouts(c, "cuda")
    bn = [dev[k].data_ptr() if c["bn"] else None for k in ("bn_w", "bn_b", "bn_m", "bn_v")]
    if "Cip" in c:
        r = lib.lseg_op_pack_conv3x3(dev["w"].data_ptr(), *bn, H.BN_EPS, dev["cb"].data_ptr() if c["cb"] else None, outs["wp"].ptr(),
                                     outs["bias"].ptr() if H.pack_has_bias(c) else None, c["Co"], c["Ci"], c["Cip"], G.LD[c["dt"]], stream())
    else:
        r = lib.lseg_op_pack_conv1x1(dev["w"].data_ptr(), *bn, H.BN_EPS, outs["wp"].ptr(), outs["bias"].ptr(), c["Co"], c["Ci"], G.LD[c["dt"]], stream())
    torch.cuda.synchronize()
    assert r == 0, f"{c['name']}: {r}: {lib.lseg_last_error(None)}"
    H.check_pack(c, d, outs)
