"""Op-level fp64 tests of the attention family through lseg_op_attention_ex, lseg_op_attention_backward_qkv and
lseg_op_attention_strict: the 2-wave and the 4-wave forward, plain and pre-scaled, both operand types and both head maps, the causal
kernel, the saved lse2, the backward on padded operands that are NOT zero, and the split-precision kernel.  Every forward case first
asserts, through lseg_op_attention_plan at this device's CU count, the variant it was written for.  References, derived bounds, guards,
padding poison, regimes and tables: tests/attention_helpers.py; tests/test_attention_family_host.py shows fp32 emulations passing and
wrong variants failing the same comparisons."""
import ctypes as C

import pytest
import torch

pytestmark = [pytest.mark.gpu, pytest.mark.gpu_fast]

from lseg_hip import _lib  # noqa: E402
import attention_helpers as A  # noqa: E402

ERR_INVALID, ERR_UNSUPPORTED = -1, -5


@pytest.fixture(scope="module")
def lib():
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    return _lib.load()


@pytest.fixture(scope="module")
def cus():
    return torch.cuda.get_device_properties(0).multi_processor_count


def P(x):
    return C.c_void_p(x if isinstance(x, int) else x.data_ptr())


def stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def assert_variant(lib, cus, c):
    r, p = A.plan(lib, c, cus)
    assert r == 0, f"{c['name']}: the plan was refused ({r})"
    if p != A.expected_plan(c):
        if cus != 256:
            pytest.skip(f"{c['name']}: written for the {c['nw']}-wave kernel at 256 CUs; {cus} CUs run {p}")
        raise AssertionError(f"{c['name']}: runs {p}, written for {A.expected_plan(c)}")


def forward(lib, cus, c, d, with_lse=True, expect=0, **over):
    """Plan, upload, launch into guarded buffers, synchronise."""
    if expect == 0:
        assert_variant(lib, cus, c)
    dev = [d[k].cuda() for k in ("qp", "kp", "vtp")]
    outs = A.make_forward_outs(c, "cuda", with_lse)
    a = dict(B=c["B"], H=c["H"], N=c["N"], npad=c["npad"], dt=A.LD[c["dt"]], causal=c["causal"], pre=c["pre"])
    a.update(over)
    r = lib.lseg_op_attention_ex(P(dev[0]), P(dev[1]), P(dev[2]), P(outs["out"].ptr()), P(outs["lse2"].ptr()) if with_lse else None, a["B"], a["H"],
                                 a["N"], a["npad"], a["dt"], a["causal"], c["scale"], a["pre"], stream())
    torch.cuda.synchronize()
    assert r == expect, f"{c['name']}: lseg_op_attention_ex returned {r}, expected {expect}: {lib.lseg_last_error(None)}"
    return outs


def run_forward(lib, cus, c):
    d = A.data(c)
    outs = forward(lib, cus, c, d)
    A.check_case(c, d, outs)
    return d, outs


@pytest.mark.parametrize("c", A.FWD2, ids=A.ids(A.FWD2))
def test_forward_two_waves(lib, cus, c):
    """Narrow grids, plain and pre-scaled: Ntok 1, 32 +- 1, 64 +- 1, 128 +- 1, 192 +- 1 (a third key tile reuses stage 0), 257; every Ntok
    with `onehot` (one wrong key costs O(1)), the other regimes in rotation, `thr` on both sides of the 2^8 refresh inside one wave."""
    run_forward(lib, cus, c)


@pytest.mark.parametrize("c", A.FWD4, ids=A.ids(A.FWD4))
def test_forward_four_waves(lib, cus, c):
    """The training forward's kernel at B >= 4 and its pre-scaled twin: B * H = 512 (head -> XCD map) at 65 and 128 tokens, 176 (map) and
    171 (plain map) at 257 tokens, where the last query block has one live wave and three that only stream."""
    run_forward(lib, cus, c)


@pytest.mark.parametrize("c", A.CAUSAL, ids=A.ids(A.CAUSAL))
def test_forward_causal(lib, cus, c):
    """`onehot` on the diagonal, just below it and on tile edges; waves whose later key tiles are wholly masked (Ntok >= 65)."""
    run_forward(lib, cus, c)


@pytest.mark.parametrize("name", ["fwd2.bf16.pre0.N65.bh3.onehot", "fwd2.f16.pre1.N129.bh3.thr", "fwd4.f16.pre0.bh176.N257.onehot+",
                                  "fwd4.bf16.pre1.bh171.N257.onehot", "causal.f16.N129.bh8.onehot"])
def test_out_is_the_same_with_and_without_lse2(lib, cus, name):
    """lse2 from both kernels is checked by every forward case; without the pointer `out` keeps its bits."""
    c = A.BY_NAME[name]
    d = A.data(c)
    a, b = forward(lib, cus, c, d, with_lse=True), forward(lib, cus, c, d, with_lse=False)
    b["out"].check(c["name"] + ".no-lse2")
    A.assert_bits_equal(a["out"].payload(), b["out"].payload(), c["name"] + ": out with and without lse2")


def backward(lib, c, d, with_ws=True, expect=0, **over):
    dev = {k: d[k].cuda() for k in ("qp", "kp", "vtp", "o", "dO", "lse2p")}
    need = lib.lseg_op_attention_backward_ws_bytes(c["B"], c["H"], c["npad"])
    outs = A.make_backward_outs(c, "cuda", ws_bytes=need if with_ws else 0)
    a = dict(npad=c["npad"], dt=A.LD[c["dt"]], N=c["N"], q=dev["qp"].data_ptr(), lse=dev["lse2p"].data_ptr())
    a.update(over)
    r = lib.lseg_op_attention_backward_qkv(P(a["q"]), P(dev["kp"]), P(dev["vtp"]), P(dev["o"]), P(dev["dO"]), P(a["lse"]) if a["lse"] else None,
                                           P(outs["dqkv"].ptr()), P(outs["ws"].ptr()) if with_ws else None, c["B"], c["H"], a["N"], a["npad"],
                                           a["dt"], c["scale"], stream())
    torch.cuda.synchronize()
    assert r == expect, f"{c['name']}: lseg_op_attention_backward_qkv returned {r}, expected {expect}: {lib.lseg_last_error(None)}"
    return outs


@pytest.mark.parametrize("c", A.BWD, ids=A.ids(A.BWD))
def test_backward(lib, cus, c):
    """dQ, dK, dV against the specified formula on the given 16-bit o and fp32 lse2, with K / V^T padding and (bounded) q / lse2 padding
    that is not zero, some dO rows all zero, the workspace supplied at exactly its stated size inside guards.  One case takes o and lse2
    from the plain forward kernel's own outputs: the pair the training step runs."""
    d = A.data(c)
    if c.get("from_forward"):
        d = dict(d)
        d.pop("_backward_reference", None)
        f = forward(lib, cus, dict(c, kind="fwd", nw=2), d)
        d["o"] = f["out"].check(c["name"] + ".forward.out").clone()
        d["lse2p"] = d["lse2p"].clone()
        d["lse2p"][:, :c["N"]] = f["lse2"].check(c["name"] + ".forward.lse2")[:, :c["N"]]
    A.check_case(c, d, backward(lib, c, d))


def test_backward_allocates_its_own_workspace(lib):
    c = A.BY_NAME["bwd.f16.N129.bh8.s0.125.onehot"]
    d = A.data(c)
    a, b = backward(lib, c, d, with_ws=True), backward(lib, c, d, with_ws=False)
    A.check_case(c, d, b, who="ws=NULL:")
    A.assert_bits_equal(a["dqkv"].payload(), b["dqkv"].payload(), c["name"] + ": dqkv with a supplied and an allocated workspace")


def test_zero_and_poisoned_padding_give_the_same_bits(lib, cus):
    """The padding contract of include/lseg_hip.h, used as far as it goes: outputs do not depend on what the padding holds."""
    c = A.TWIN_FWD
    outs = [forward(lib, cus, x, A.data(x)) for x in (c, dict(c, poison=False))]
    A.assert_bits_equal(outs[0]["out"].payload(), outs[1]["out"].payload(), c["name"] + ".out zero vs poisoned padding")
    A.assert_bits_equal(outs[0]["lse2"].payload()[:, :c["N"]], outs[1]["lse2"].payload()[:, :c["N"]], c["name"] + ".lse2 zero vs poisoned padding")
    c = A.TWIN_BWD
    outs = [backward(lib, x, A.data(x)) for x in (c, dict(c, poison=False))]
    A.assert_bits_equal(outs[0]["dqkv"].payload(), outs[1]["dqkv"].payload(), c["name"] + ".dqkv zero vs poisoned padding")


@pytest.mark.parametrize("c", A.STRICT, ids=A.ids(A.STRICT))
def test_strict(lib, c):
    """The split-precision kernel on hi + lo planes: Ntok 1 and 3 leave key partitions empty, `low` keeps every score far below zero."""
    d = A.data(c)
    dev = [d[k].cuda() for k in ("qp", "kp", "vtp")]
    outs = A.make_strict_outs(c, "cuda")
    plane = c["BH"] * c["npad"] * 64
    r = lib.lseg_op_attention_strict(P(dev[0]), P(dev[1]), P(dev[2]), P(outs["out"].ptr()), plane, plane, c["B"] * c["N"] * c["H"] * 64, c["B"],
                                     c["H"], c["N"], c["npad"], c["scale"], stream())
    torch.cuda.synchronize()
    assert r == 0, lib.lseg_last_error(None)
    A.check_case(c, d, outs)


def test_refusals_by_return_code(lib, cus):
    c = A.BY_NAME["fwd2.bf16.pre0.N65.bh3.onehot"]
    d = A.data(c)
    for over, code in ((dict(npad=192), ERR_INVALID), (dict(npad=0), ERR_INVALID), (dict(N=129), ERR_INVALID), (dict(pre=1, causal=1), ERR_UNSUPPORTED),
                       (dict(dt=_lib.LSEG_F32), ERR_INVALID), (dict(B=0), ERR_INVALID), (dict(N=0), ERR_INVALID)):
        outs = forward(lib, cus, c, d, expect=code, **over)
        outs["out"].untouched(f"{c['name']} {over}")
        outs["lse2"].untouched(f"{c['name']} {over}")
    q = d["qp"].cuda()
    out = A.make_forward_outs(c, "cuda")["out"]
    for ptrs in ((None, P(q), P(q), P(out.ptr())), (P(q), None, P(q), P(out.ptr())), (P(q), P(q), None, P(out.ptr())), (P(q), P(q), P(q), None)):
        assert lib.lseg_op_attention_ex(*ptrs, None, c["B"], c["H"], c["N"], c["npad"], A.LD["bf16"], 0, c["scale"], 0, stream()) == ERR_INVALID
        assert lib.lseg_op_attention_strict(*ptrs, 0, 0, 0, c["B"], c["H"], c["N"], c["npad"], c["scale"], stream()) == ERR_INVALID
    torch.cuda.synchronize()
    out.untouched(c["name"] + " NULL operands")
    c = A.TWIN_BWD
    d = A.data(c)
    q = d["qp"].cuda()
    for over in (dict(npad=192), dict(N=129), dict(dt=_lib.LSEG_F32), dict(q=q.data_ptr() + 2), dict(lse=0), dict(N=0)):
        outs = backward(lib, c, d, expect=ERR_INVALID, **over)
        outs["dqkv"].untouched(f"{c['name']} {over}")
