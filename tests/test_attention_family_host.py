"""Host self-check of the attention family's op-level tests (no GPU): plain fp32 torch emulations of the kernels' arithmetic pass every
case of every table through the check functions of tests/attention_helpers.py (the bounds are not too tight), wrong variants of those
emulations fail the same comparisons on named cases of the GPU tables (the bounds and the data are not too loose), the launcher's plan
gives every case the kernel variant it was written for, and the backward formula is fp64 autograd."""
import pytest
import torch

from lseg_hip import _lib
import attention_helpers as A

ERR_INVALID, ERR_UNSUPPORTED = -1, -5


@pytest.fixture(scope="module")
def lib():
    return _lib.load()


def _data(c):
    d = A.data(c)
    if c.get("from_forward"):                  # o and lse2 from the forward emulation's own outputs, as the training step pairs the kernels
        d = dict(d)
        d.pop("_backward_reference", None)
        f = A.emulate_forward(dict(c, kind="fwd", nw=2), d)
        d["o"] = f["out"].payload().clone()
        d["lse2p"] = d["lse2p"].clone()
        d["lse2p"][:, :c["N"]] = f["lse2"].payload()[:, :c["N"]]
    return d


@pytest.mark.parametrize("c", A.ALL, ids=A.ids(A.ALL))
def test_emulation_is_accepted(c):
    d = _data(c)
    A.check_case(c, d, A.emulate(c, d), who="emu:")


# wrong variant -> the named cases of the GPU tables that must reject it
WRONG = {
    "drop-last-key": ["fwd2.bf16.pre0.N65.bh3.onehot", "fwd2.f16.pre1.N128.bh8.onehot", "fwd4.bf16.pre0.bh176.N257.onehot+",
                      "causal.f16.N129.bh3.onehot"],
    "key-ntok": ["fwd2.bf16.pre0.N1.bh8.plain.s0.2", "fwd2.bf16.pre1.N1.bh3.low", "fwd2.bf16.pre0.N33.bh3.low"],
    "causal-lt": ["causal.bf16.N1.bh3.onehot", "causal.f16.N77.bh8.onehot"],
    "kv-end-short": ["causal.bf16.N129.bh3.onehot", "causal.f16.N200.bh8.onehot"],
    "no-rescale": ["fwd2.bf16.pre0.N129.bh3.thr", "causal.bf16.N200.bh3.spike"],
    "refresh-l-not-o": ["fwd2.bf16.pre1.N129.bh3.thr", "fwd2.f16.pre1.N193.bh3.thr"],
    "first-ref-0": ["fwd2.bf16.pre1.N33.bh3.low", "fwd2.f16.pre1.N33.bh3.low"],
    "lse-no-max": ["fwd2.bf16.pre0.N65.bh3.onehot", "fwd2.f16.pre1.N65.bh8.onehot"],
    "lse-pad-rows": ["fwd2.bf16.pre0.N65.bh3.onehot", "fwd2.bf16.pre1.N129.bh3.onehot"],
    "heads-swapped": ["fwd4.bf16.pre0.bh176.N257.onehot+", "fwd2.f16.pre1.N128.bh8.onehot"],
    "stage-early": ["fwd2.bf16.pre0.N129.bh8.onehot", "fwd2.f16.pre1.N193.bh8.onehot", "fwd4.bf16.pre1.bh176.N257.onehot+"],
    "dq-no-tail-mask": ["bwd.bf16.N65.bh8.s0.2.onehot", "bwd.f16.N129.bh8.s0.125.onehot"],
    "dk-no-scale": ["bwd.bf16.N65.bh8.s0.2.onehot", "bwd.f16.N64.bh8.s0.125.onehot"],
    "D-from-dOdO": ["bwd.bf16.N65.bh3.s0.125.plain", "bwd.f16.N257.bh8.s0.125.onehot"],
    "empty-partition": ["strict.N1.low", "strict.N3.low"],
}


@pytest.mark.parametrize("wrong,name", [(w, n) for w, ns in WRONG.items() for n in ns])
def test_wrong_variant_is_rejected(wrong, name):
    c = A.BY_NAME[name]
    d = _data(c)
    with pytest.raises(AssertionError):
        A.check_case(c, d, A.emulate(c, d, wrong=wrong), who=f"wrong[{wrong}]:")


def test_missing_tail_mask_hides_behind_zero_padding():
    """The point of the padding poison: with zero K padding the dQ kernel's missing tail mask multiplies by a zero K^T column and passes."""
    c = dict(A.TWIN_BWD, poison=False)
    d = A.data(c)
    A.check_case(c, d, A.emulate(c, d, wrong="dq-no-tail-mask"), who="zero-padded wrong[dq-no-tail-mask]:")
    c = A.TWIN_BWD
    with pytest.raises(AssertionError):
        A.check_case(c, A.data(c), A.emulate(c, A.data(c), wrong="dq-no-tail-mask"), who="poisoned wrong[dq-no-tail-mask]:")


@pytest.mark.parametrize("c0", [A.TWIN_FWD, A.TWIN_BWD], ids=lambda c: c["name"])
def test_emulated_twins_are_bit_equal(c0):
    """Zero padding and poisoned padding give the same bits (the emulation walks the padded rows as the kernels do)."""
    outs = [A.emulate(c, A.data(c)) for c in (c0, dict(c0, poison=False))]
    for k in ("out", "dqkv"):
        if k in outs[0]:
            A.assert_bits_equal(outs[0][k].payload(), outs[1][k].payload(), f"{c0['name']}.{k} zero vs poisoned padding")


def test_every_case_runs_its_variant_at_256_cus(lib):
    for c in A.FWD2 + A.FWD4 + A.CAUSAL:
        r, p = A.plan(lib, c, 256)
        assert r == 0 and p == A.expected_plan(c), f"{c['name']}: plan {p} (status {r}), written for {A.expected_plan(c)}"
    kinds = {(c["dt"], c["nw"], c["pre"], c["causal"]) for c in A.FWD2 + A.FWD4 + A.CAUSAL}
    assert kinds == {(dt, nw, pre, 0) for dt in ("bf16", "f16") for nw in (2, 4) for pre in (0, 1)} | {(dt, 4, 0, 1) for dt in ("bf16", "f16")}
    assert {c["BH"] % 8 == 0 for c in A.FWD4} == {True, False}


def test_variants_at_64_cus(lib):
    """On a 64-CU device 2 * CUs = 128 workgroups fill the chip: which cases of the tables would run another variant there."""
    changed = []
    for c in A.FWD2 + A.FWD4 + A.CAUSAL:
        r, p = A.plan(lib, c, 64)
        assert r == 0
        narrow = -(-c["N"] // 128) * c["BH"] < 128 and not c["causal"]
        assert p[0] == (2 if narrow else 4), c["name"]
        if p[0] != c["nw"]:
            changed.append(c["name"])
    print(f"attention plan at 64 CUs: {len(changed)} cases change variant: {changed}")
    assert changed == [], "every table entry is narrow (B * H <= 8) or wide (>= 171 workgroups per query block row) on both chips"


def test_plan_refusals(lib):
    import ctypes as C
    out6 = (C.c_int * 6)()
    assert lib.lseg_op_attention_plan(1, 2, 77, 1, 1, 256, C.byref(out6)) == ERR_UNSUPPORTED          # prescaled with causal
    for B, H, N, cus in ((0, 1, 1, 256), (1, 0, 1, 256), (1, 1, 0, 256), (1, 1, 1, 0)):
        assert lib.lseg_op_attention_plan(B, H, N, 0, 0, cus, C.byref(out6)) == ERR_INVALID
    assert lib.lseg_op_attention_plan(1, 1, 1, 0, 0, 256, None) == ERR_INVALID
    # the boundary of `narrow`: ceil(ntok / 128) B H < 2 cus
    for bh, want in ((511, 2), (512, 4)):
        assert lib.lseg_op_attention_plan(1, bh, 128, 0, 0, 256, C.byref(out6)) == 0 and out6[0] == want
    assert lib.lseg_op_attention_plan(1, 2, 901, 0, 1, 256, C.byref(out6)) == 0 and tuple(out6) == (2, 15, 30, 15, 0, 32768)
    assert lib.lseg_op_attention_plan(36, 16, 901, 0, 1, 256, C.byref(out6)) == 0 and tuple(out6) == (4, 8, 4608, 15, 1, 32768)


def test_formula_equals_autograd():
    assert A.formula_equals_autograd() < 1e-12


def test_regimes_do_what_they_say():
    """onehot puts nearly all weight on the designated key, and the designated keys include the edges; thr straddles 2^8 inside a wave."""
    c = A.BY_NAME["fwd2.bf16.pre1.N129.bh3.onehot"]
    d = A.data(c)
    P = torch.softmax((d["q"].double() @ d["k"].double().transpose(1, 2)) * A.LN2, -1)
    tgt = A.onehot_targets(c["N"], 0)
    assert (P[:, torch.arange(c["N"]), tgt] > 0.99).all()
    assert {0, 63, 64, 127, 128}.issubset(set(tgt.tolist()))
    ct = A.onehot_targets(200, 1)
    assert all(int(ct[i]) <= i for i in range(200)) and any(int(ct[i]) == i for i in range(1, 200)) and any(int(ct[i]) == i - 1 for i in range(1, 200))
    c = A.BY_NAME["fwd2.f16.pre1.N129.bh3.thr"]
    d = A.data(c)
    s = d["q"].double() @ d["k"].double().transpose(1, 2)
    rel = s[:, :, 64:128].amax(-1) - s[:, :, :64].amax(-1)
    for lane, (lo, hi) in enumerate(((7.0, 8.0), (8.0, 9.0), (-1.0, 1.0), (-4.0, -2.0))):
        assert ((rel[:, lane::4] > lo) & (rel[:, lane::4] < hi)).all(), lane
