"""Op-level fp64 tests of the GEMM family (csrc/gemm.hip) through lseg_op_gemm_ex, which builds its arguments with the builders the
schedules use (csrc/engine.h): every specialised epilogue at every tile it is instantiated for and both operand types, the persistent
XCD-sliced schedule with 1 .. 6 work items per workgroup over 1 .. 5 K-steps (the A cursor crosses a tile boundary up to every step),
ragged tile counts, a short last rasterisation group, split-K with a short last range, GELU over its whole domain, the pixel-shuffle
ConvTranspose and the periodic patch-embed rows.  Every case first asserts, through lseg_op_gemm_ex_plan at this device's CU count,
that it runs the epilogue, the tile and the work items per workgroup it was written for.  References, counted bounds, intervals and
guarded buffers: tests/gemm_helpers.py; tests/test_gemm_family_host.py shows wrong variants failing the same comparisons."""
import ctypes as C

import pytest
import torch

pytestmark = [pytest.mark.gpu, pytest.mark.gpu_fast]

from lseg_hip import _lib  # noqa: E402
import gemm_helpers as G  # noqa: E402

ERR_INVALID = -1


@pytest.fixture(scope="module")
def lib():
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    return _lib.load()


@pytest.fixture(scope="module")
def cus():
    return torch.cuda.get_device_properties(0).multi_processor_count


def launch(lib, cus, c, d, fill=None, expect=0, **over):
    """Upload, plan, launch into guarded buffers, synchronise.  The device tensors live until the synchronise."""
    dev = {k: d[k].cuda() for k in ("A", "W", "bias", "res") if k in d}
    outs = G.make_outs(c, d, "cuda", fill=fill)
    ptrs = {k: t.data_ptr() for k, t in dev.items()}
    ptrs.setdefault("res", 0)
    for k in ("C", "Ck", "Cv"):
        ptrs[k] = outs[k].ptr() if k in outs else 0
    g = G.struct_of(c, d, ptrs)
    for k, v in over.items():
        setattr(g, k, v)
    if expect == 0:
        G.assert_plan(lib, c, g, cus)
    r = lib.lseg_op_gemm_ex(C.byref(g), C.c_void_p(torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    assert r == expect, f"{c['name']}: lseg_op_gemm_ex returned {r}, expected {expect}: {lib.lseg_last_error(None)}"
    return outs


def run(lib, cus, c):
    d = G.data(c)
    outs = launch(lib, cus, c, d)
    G.check_case(c, d, outs)
    return d, outs


@pytest.mark.parametrize("c", G.SCHEDULE, ids=G.ids(G.SCHEDULE))
def test_schedule_and_ring_cursors(lib, cus, c):
    """a. nk in 1..5 K-steps x 1, 2, 3, 4, 6 tiles per workgroup (max_grid = 8, one workgroup per XCD) on 64x64 and 128x128 tiles, M ragged;
    8 t + 3 tiles, fewer than 8 tiles, an 11 x 3 tile grid (last rasterisation group of 3 row-blocks), 256x256 at the natural grid."""
    run(lib, cus, c)


@pytest.mark.parametrize("c", G.SPLITK, ids=G.ids(G.SPLITK))
def test_split_k(lib, cus, c):
    """b. EPI_PART32 with a short last range, ranges of one step, two uneven ranges; two or three (tile, K-range) items per workgroup.
    Each slab against the fp64 partial sum of its own K-range, the fp64 sum of the slabs against the whole product, the slab behind the
    last one untouched."""
    run(lib, cus, c)


def test_split_k_ranges_that_do_not_tile_K_are_refused(lib, cus):
    c = next(x for x in G.SPLITK if x["name"] == "splitk.t2.nk5.3x2.bf16")
    d = G.data(c)
    for over in (dict(split_steps=1), dict(nsplit=4), dict(nsplit=6, split_steps=1), dict(split_steps=3), dict(split_steps=0)):
        outs = launch(lib, cus, c, d, expect=ERR_INVALID, **over)
        outs["C"].untouched(f"{c['name']} {over}")


@pytest.mark.parametrize("c", G.EPILOGUE, ids=G.ids(G.EPILOGUE))
def test_epilogues(lib, cus, c):
    """c. LIN16, LIN16_GELU (both symbols), LIN16_F16, LIN32, RES32 (in place), QKV16 (plain and with q pre-scaled) x tile 1, 2, 6 x bf16,
    fp16 at M = 37 and 203; 256x256 asked for at N = 384 falls back to 128x128; the generic epilogue at N = 200 and at a C pointer
    8 bytes off meets the same bound."""
    run(lib, cus, c)


@pytest.mark.parametrize("c", G.GELU_DOMAIN, ids=G.ids(G.GELU_DOMAIN))
def test_gelu_over_its_whole_domain(lib, cus, c):
    """d. K = 64 against an identity: the accumulator IS the operand value.  Every bf16 / fp16 value in [-12, 12], both zeros, the largest
    finite value and its negative, against fp64 x Phi(x) within gelu_fast's stated error and its stated -3e-10 |x| tail."""
    d, outs = run(lib, cus, c)
    x = d["A"].reshape(-1)
    y = outs["C"].payload()[:x.numel() // 64, :64].reshape(-1).cpu()
    zero = x.float() == 0
    assert (y[zero].float() == 0).all(), "gelu(+-0) is not a zero"
    assert (outs["C"].payload()[:x.numel() // 64, 64:] == 0).all(), "the zero columns of W give a non-zero output"


@pytest.mark.parametrize("c", G.PIXSHUF, ids=G.ids(G.PIXSHUF))
def test_pixel_shuffle_conv_transpose(lib, cus, c):
    """e. against F.conv_transpose2d in fp64; the one-pixel border keeps its pattern; every interior cell is written exactly once: a
    second run into a map pre-filled with another value gives the same bits."""
    d, outs = run(lib, cus, c)
    again = launch(lib, cus, c, d, fill=3.0)
    again["C"].check(c["name"] + ".second")
    m = outs["C"].must
    G.assert_bits_equal(again["C"].payload()[m], outs["C"].payload()[m], c["name"] + ".second")


@pytest.mark.parametrize("c", G.PERIODIC, ids=G.ids(G.PERIODIC))
def test_periodic_patch_embed_rows(lib, cus, c):
    """f. rows b * ntok + p + 1 = patches + bias + pos[p + 1] against cat(cls, patches) + pos; row 0 of every image keeps its pattern."""
    run(lib, cus, c)
