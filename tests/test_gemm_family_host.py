"""Host-side self-check of tests/gemm_helpers.py and of the launcher's choices: a plain fp32 torch emulation of every form passes the
comparisons tests/test_gpu_gemm_family.py uses, wrong variants fail them -- through the same functions --, the launcher's plan names
the epilogue, the tile and the work items per workgroup every GPU case was written for (at 256 and at 64 compute units), and
lseg_op_gemm_ex refuses malformed cases by return code.  Needs no GPU."""
import ctypes as C

import pytest
import torch

import gemm_helpers as G
from lseg_hip import _lib

ERR_INVALID, ERR_UNSUPPORTED = -1, -5


@pytest.fixture(scope="module")
def lib():
    return _lib.load()


def rejected(what, c, d, wrong):
    with pytest.raises(AssertionError) as e:
        G.check_case(c, d, G.emulate(c, d, wrong), who="host.wrong.")
    print(f"wrong-variant {what} [{c['name']}]: {str(e.value).splitlines()[0]}")


def by_name(name):
    return next(c for c in G.ALL if c["name"] == name)


# ---- the rounding and the GELU range ---------------------------------------------------------------------------------------------------------
def test_round_to_rounds_once_to_nearest_even():
    x = torch.randn(20000, generator=torch.Generator().manual_seed(1)) * torch.logspace(-42, 38, 20000)
    assert torch.equal(G.round_to(x.double(), "bf16"), x.bfloat16().double())          # fp32 -> bf16 is one rounding in torch as well
    assert torch.equal(G.round_to(x.double(), "f16"), x.half().double())
    d = torch.tensor([1 + 2.0 ** -8 + 2.0 ** -40, 1 + 2.0 ** -8, 1 + 3 * 2.0 ** -8, 3.4e38, -3.4e38, 0.0], dtype=torch.float64)
    want = torch.tensor([1 + 2.0 ** -7, 1.0, 1 + 2.0 ** -6, float("inf"), float("-inf"), 0.0], dtype=torch.float64)
    assert torch.equal(G.round_to(d, "bf16"), want)                                  # above a tie: up (through fp32 it would land on the tie); ties to even
    assert G.round_to(torch.tensor([1 + 2.0 ** -11 + 2.0 ** -30], dtype=torch.float64), "f16").item() == 1 + 2.0 ** -10


def test_gelu_range_holds_the_minimum_and_the_tail():
    x = torch.linspace(-12, 12, 240001, dtype=torch.float64)
    g = G.gelu64(x)
    i = int(g.argmin())
    assert abs(x[i].item() - G.GELU_MIN_X) < 2e-4 and abs(g[i].item() + 0.16997120) < 1e-7
    lo, hi = G.act_range(torch.tensor([-1.0, -9.0, 0.5], dtype=torch.float64), torch.tensor([-0.5, -8.0, 0.6], dtype=torch.float64), G.ACT_GELU)
    assert lo[0] < g[i] and lo[0] > g[i] - 1e-6 and hi[0] >= G.gelu64(torch.tensor(-1.0, dtype=torch.float64))
    assert -4.6e-7 - 3.1e-9 < lo[1] < -4.6e-7 - 2.7e-9 and 0 < hi[1] < 4.7e-7        # the stated 4.6e-7 either way, -3e-10 * 9 more below
    assert lo[2] < G.gelu64(torch.tensor(0.5, dtype=torch.float64)) < G.gelu64(torch.tensor(0.6, dtype=torch.float64)) < hi[2]


def test_gelu_domain_holds_every_operand_value():
    for ab, n_pos in (("bf16", 0x4140 + 1), ("f16", 0x4A00 + 1)):                     # bit patterns 0 .. that of 12.0
        v = G.gelu_domain_values(ab).reshape(-1)
        assert len(set(v.view(torch.int16).tolist())) == 2 * n_pos + 2                 # +-[0, 12] and the two largest finite values
        f = v.float()
        assert (f == torch.finfo(G.TD[ab]).max).any() and (f == -torch.finfo(G.TD[ab]).max).any()
        assert ((f > 6.2) & (f < G.GELU_KNEE)).any() and ((f > G.GELU_KNEE) & (f <= 6.25)).any()


# ---- the emulation passes, the wrong variants fail ---------------------------------------------------------------------------------------------
HOST_PASS = ([c for c in G.SCHEDULE if ".x1." in c["name"] or ".x6." in c["name"] or ".nk" not in c["name"]] + G.SPLITK
             + [c for c in G.EPILOGUE if "M37" not in c["name"]] + G.GELU_DOMAIN + G.PIXSHUF + G.PERIODIC)


@pytest.mark.parametrize("c", HOST_PASS, ids=G.ids(HOST_PASS))
def test_fp32_emulation_passes(c):
    d = G.data(c)
    G.check_case(c, d, G.emulate(c, d), who="host.")


LINEAR_WRONG = ["sched.t1.nk1.x3.bf16.LIN32", "sched.t2.nk3.x2.f16.GENERIC", "sched.t1.11x3.f16", "sched.t6.natural.bf16", "epi.LIN16.t2.M203.bf16",
                "epi.LIN32.t1.M203.f16", "epi.RES32.t6.M203.bf16", "epi.F16.t1.M203.bf16", "epi.GELU.t2.M203.f16",
                "epi.generic-of-LIN16.N200.t1.bf16", "epi.generic-of-RES32.C+8B.t2.f16"]


@pytest.mark.parametrize("name", LINEAR_WRONG)
def test_linear_wrong_variants_fail(name):
    c = by_name(name)
    d = G.data(c)
    if c["K"] > 64:                                                  # at K = 64 the only K-step is the last one: an all-zero product
        rejected("last K-step dropped", c, d, "drop-last-k")
    else:
        rejected("the only K-step dropped", c, d, "drop-last-k")
    if G.rows(c, d) > G._tile_rows(c):
        rejected("first K-step from the next row-tile", c, d, "next-tile-k0")
    if c["bias"]:
        rejected("bias shifted by four columns", c, d, "bias+4")
    rejected("last ragged row one row down", c, d, "last-row-down")
    if c["act"] == G.ACT_GELU:
        rejected("ReLU in place of GELU", c, d, "relu-for-gelu")


@pytest.mark.parametrize("c", [c for c in G.SPLITK if ".bf16" in c["name"]], ids=lambda c: c["name"])
def test_splitk_wrong_variants_fail(c):
    d = G.data(c)
    rejected("short split-K range counted twice", c, d, "short-range-twice")
    rejected("last K-step of every range dropped", c, d, "drop-last-k")
    rejected("first K-step from the next row-tile", c, d, "next-tile-k0")
    rejected("last ragged row one row down", c, d, "last-row-down")
    rejected("k_beg / k_end kept from the previous K-range", c, d, "stale-range")


@pytest.mark.parametrize("c", G.SPLITK, ids=G.ids(G.SPLITK))
def test_splitk_workgroups_move_between_k_ranges(c):
    """The kernel's own slicing of every split-K case: each workgroup walks at least two work items, and for every boundary between two
    K-ranges some workgroup walks across it -- into the short last range too (3 x 2 of 5 steps, 2 x 3 of 5 steps)."""
    slices = G.splitk_slices(c)
    assert len(slices) == 8 and min(len(w) for w in slices) >= 2 and max(len(w) for w in slices) == c["exp"][2]
    flat = sorted(it for w in slices for it in w)
    assert len(flat) == len(set(flat)) == c["nsplit"] * len({it[1:] for it in flat})         # every (range, tile) pair exactly once
    crossed = {(a[0], b[0]) for w in slices for a, b in zip(w, w[1:]) if a[0] != b[0]}
    assert crossed == {(s, s + 1) for s in range(c["nsplit"] - 1)}, crossed
    nk, ns, st = c["K"] // 64, c["nsplit"], c["steps"]
    if nk - (ns - 1) * st < st:
        assert (ns - 2, ns - 1) in crossed                        # from a full range into the short one: k_end changes, not only k_beg


@pytest.mark.parametrize("name", ["epi.QKV16.t2.plain.bf16", "epi.QKV16.t1.scaled.f16", "epi.QKV16.t6.scaled.bf16"])
def test_qkv_wrong_variants_fail(name):
    c = by_name(name)
    d = G.data(c)
    rejected("last K-step dropped", c, d, "drop-last-k")
    rejected("bias shifted by four columns", c, d, "bias+4")
    rejected("last token one row down (a pad token)", c, d, "last-row-down")
    if c["exp"][1] == 1:
        rejected("first K-step from the next row-tile", c, d, "next-tile-k0")
    if c["qscale"]:
        rejected("q scaled after the rounding", c, d, "scale-after-rounding")


@pytest.mark.parametrize("c", [c for c in G.GELU_DOMAIN], ids=lambda c: c["name"])
def test_gelu_domain_wrong_variants_fail(c):
    d = G.data(c)
    rejected("ReLU in place of GELU", c, d, "relu-for-gelu")
    rejected("the only K-step dropped", c, d, "drop-last-k")


@pytest.mark.parametrize("name", ["pixshuf.s2.ch64.t1.bf16", "pixshuf.s4.ch32.t2.f16", "pixshuf.s2.ch128.t6.bf16", "pixshuf.s2.ch24.generic.f16"])
def test_pixshuf_wrong_variants_fail(name):
    c = by_name(name)
    d = G.data(c)
    rejected("sub-pixel (i, j) transposed", c, d, "ij-transposed")
    rejected("last K-step dropped", c, d, "drop-last-k")
    rejected("bias shifted by four channels", c, d, "bias+4")
    rejected("last pixel one map row down (the border)", c, d, "last-row-down")


@pytest.mark.parametrize("c", [c for c in G.PERIODIC if ".t1." in c["name"]], ids=lambda c: c["name"])
def test_periodic_wrong_variants_fail(c):
    d = G.data(c)
    rejected("p_off = 0 (the cls rows written, pos rows one up)", c, d, "p_off=0")
    rejected("bias shifted by four columns", c, d, "bias+4")
    rejected("an image's last patch one row down (the next cls row)", c, d, "last-row-down")
    rejected("last K-step dropped" if c["K"] > 64 else "the only K-step dropped", c, d, "drop-last-k")
    if G.rows(c, d) > G._tile_rows(c):                            # 2 x 36 rows on 64-row tiles; the pixel-shuffle cases (M = 30) have one row-tile
        rejected("first K-step from the next row-tile", c, d, "next-tile-k0")


# ---- the plan ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cus", [256, 64])
def test_every_gpu_case_runs_what_it_was_written_for(lib, cus):
    for c in G.ALL:
        p = G.assert_plan(lib, c, G.struct_of(c, G.data(c) if c["M"] is None else None), cus)
        assert p[2] % 8 == 0 and p[2] >= 8
        if c["max_grid"]:
            assert p[2] == c["max_grid"], c["name"]
    items = {c["exp"][2] for c in G.SCHEDULE if ".nk" in c["name"]}
    assert items == {1, 2, 3, 4, 6}
    assert {c["exp"][1] for c in G.ALL} == {1, 2, 6}
    assert {c["exp"][0] for c in G.ALL} == set(G.EPI.values())


def test_tile_hint_one_is_honoured_and_the_cost_model_is_unchanged(lib):
    c = dict(by_name("epi.LIN16.t1.M203.bf16"), M=36 * 901, N=4096, K=1024, tile=0)
    assert G.plan(lib, G.struct_of(c, None), 256)[1][1] == 6           # the ViT-L fc1 at B = 36: 256 x 256 by the cost model
    assert G.plan(lib, G.struct_of(dict(c, tile=1), None), 256)[1][1] == 1
    assert G.plan(lib, G.struct_of(dict(c, tile=2), None), 256)[1][1] == 2
    small = dict(c, M=203, N=256, K=192)
    assert G.plan(lib, G.struct_of(small, None), 256)[1][1] == 1         # fewer than 192 mid tiles: 64 x 64
    r, p = G.plan(lib, G.struct_of(c, None), 256)
    assert p[2] == 256 and p[3] == -(-(-(-36 * 901 // 256) * 16) // 8 // 32)   # one 8-wave workgroup per CU; ceil(ceil(tiles / 8) / (grid / 8))


# ---- refusals, by return code, before any launch (and before a device is asked for) --------------------------------------------------
def test_malformed_cases_are_refused(lib):
    base = by_name("epi.LIN16.t2.M203.bf16")

    def code(c, **over):
        g = G.struct_of(c, None)
        for k, v in over.items():
            setattr(g, k, v)
        r1 = lib.lseg_op_gemm_ex(C.byref(g), None)
        r2, _ = G.plan(lib, g, 256)
        assert r1 == r2, (over, r1, r2)
        return r1

    assert lib.lseg_op_gemm_ex(None, None) == ERR_INVALID
    assert lib.lseg_op_gemm_ex_plan(C.byref(G.struct_of(base, None)), 256, None) == ERR_INVALID
    assert G.plan(lib, G.struct_of(base, None), 0)[0] == ERR_INVALID
    for over in (dict(A=None), dict(W=None), dict(C=None), dict(M=0), dict(N=-1), dict(form=4), dict(tag=2), dict(tile=3), dict(tile=5),
                 dict(max_grid=12), dict(max_grid=-8), dict(act=2), dict(ab_dtype=_lib.LSEG_F32), dict(out_dtype=7), dict(nsplit=-1)):
        assert code(base, **over) == ERR_INVALID, over
    assert code(base, K=100) == ERR_UNSUPPORTED                        # launch_gemm: K % 64
    # split-K ranges that do not tile K exactly, or a bias beside them: launch_gemm's refusals
    sk = by_name("splitk.t2.nk5.3x2.bf16")
    assert G.plan(lib, G.struct_of(sk, None), 256)[0] == 0
    for over in (dict(split_steps=1), dict(nsplit=4), dict(nsplit=6, split_steps=1), dict(split_steps=0), dict(split_steps=3),
                 dict(bias=G.FAKE + 0x200000), dict(residual=G.FAKE + 0x300000)):
        assert code(sk, **over) == ERR_INVALID, over
    q = by_name("epi.QKV16.t2.scaled.bf16")
    for over in (dict(heads=3), dict(K=192), dict(N=512), dict(ntok=0), dict(npad=36), dict(M=110), dict(Ck=None), dict(Cv=None), dict(bias=None),
                 dict(act=1), dict(residual=G.FAKE)):
        assert code(q, **over) == ERR_INVALID, over
    assert code(q, Ck=G.FAKE + 8) == ERR_UNSUPPORTED                  # qscale without the specialised epilogue
    px = by_name("pixshuf.s2.ch64.t2.bf16")
    for over in (dict(s=0), dict(ch=32), dict(M=31), dict(ho=0), dict(N=128), dict(bias=None)):
        assert code(px, **over) == ERR_INVALID, over
    pe = by_name("periodic.3x9.D128.t1.bf16")
    for over in (dict(residual=None), dict(p_div=0), dict(p_off=-1), dict(p_mul=9), dict(M=28), dict(ldr=64)):
        assert code(pe, **over) == ERR_INVALID, over


def test_struct_mirror_matches_the_header():
    import os
    import re
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "lseg_hip.h")).read()
    body = hdr.split("typedef struct lseg_gemm_case {")[1].split("} lseg_gemm_case;")[0]
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    names = []
    for decl in body.split(";"):
        decl = decl.strip()
        if decl:
            names += [re.sub(r"[^A-Za-z0-9_]", "", part.split()[-1]) for part in decl.split(",")]
    assert names == [f[0] for f in _lib.LSegGemmCase._fields_]
