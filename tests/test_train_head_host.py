"""The plan of the training step's label head (csrc/train_head.h, through lseg_op_train_head_plan: host only, no device) against a
transcription of the conditions the training step had before they were gathered there -- csrc/train.hip at commit cd90f6d, cited by
line, with check_grouping (engine.hip:670-675) and check_ragged_train (forward_request.hip:66-72) -- over the full cross product of
groupings, label counts, head blocks, gradient precisions and the LSEG_CORR_RAGGED_GEMM switch."""
import ctypes as C

import numpy as np

from lseg_hip import _lib

ERR_INVALID, ERR_UNSUPPORTED = -1, -5
SHARED, GROUPED, RAGGED_GEMM, RAGGED_FUSED = range(4)
NO_REFUSAL, HEAD_BLOCKS_REFUSED, RAGGED_LOGITS, GROUP_SIZE = range(4)         # which refusal: the first that held in the parent's order
F16, BF16 = 1, 2

COLS = ["group_k", "ragged", "kmax", "K", "hb_n", "arch_option", "unrounded", "img_dt", "out_c", "logits", "ragged_gemm"]
RAGGED = [(0, 0), (1, 1), (1, 5), (1, 64), (1, 65), (1, 200)]                    # (lists set, the longest list)
HEAD_BLOCKS = [(0, 0), (1, 1), (1, 2), (2, 1), (2, 2)]                          # (blocks, arch_option): none without an arch_option


def up64(v):
    return (v + 63) // 64 * 64


def product_rows():
    axes = [(0, 1, 3, 8, 9), range(len(RAGGED)), (1, 5, 64, 65, 150), range(len(HEAD_BLOCKS)), (0, 1), (F16, BF16), (64, 128, 100), (0, 1), (0, 1)]
    gk, rag, K, hb, unr, dt, out_c, logits, sw = np.array(np.meshgrid(*axes, indexing="ij")).reshape(len(axes), -1).astype(np.int64)
    rg, hbs = np.array(RAGGED), np.array(HEAD_BLOCKS)
    return dict(group_k=gk, ragged=rg[rag, 0], kmax=rg[rag, 1], K=K, hb_n=hbs[hb, 0], arch_option=hbs[hb, 1], unrounded=unr, img_dt=dt,
                out_c=out_c, logits=logits, ragged_gemm=sw)


def call_entry(v):
    n = len(v["K"])
    rows = np.ascontiguousarray(np.stack([v[c] for c in COLS], axis=1).astype(np.int32))
    out = np.full((n, 8), -99, np.int32)
    assert _lib.load().lseg_op_train_head_plan(rows.ctypes.data_as(C.c_void_p), n, out.ctypes.data_as(C.c_void_p)) == 0
    return out


def parent_conditions(v):
    """(status, mode, kout, Kp, hdt, dgrad operand, head blocks, which refusal) per row.  First true refusal wins, in the order the
    parent met them."""
    gk, K, kmax, out_c, arch = v["group_k"], v["K"], v["kmax"], v["out_c"], v["arch_option"]
    rag, logits, sw, unr = (v[k].astype(bool) for k in ("ragged", "logits", "ragged_gemm", "unrounded"))
    group_ok = (gk >= 1) & (gk <= 8) & (out_c >= 8) & (out_c % 8 == 0) & (out_c <= 1024)         # corr_group.hip:191
    refusal = np.select([
        rag & (arch != 0),                   # forward_request.hip:67 (check_request, before forward_train)
        (gk > 0) & (arch != 0),              # train.hip:479 -> engine.hip:673
        rag & logits,                        # train.hip:482
        (gk > 0) & ~group_ok,                # train.hip:484
    ], [HEAD_BLOCKS_REFUSED, HEAD_BLOCKS_REFUSED, RAGGED_LOGITS, GROUP_SIZE], NO_REFUSAL)
    status = np.where(refusal != NO_REFUSAL, ERR_UNSUPPORTED, 0)                                 # all four: LSEG_ERR_UNSUPPORTED
    mode = np.select([rag & sw, rag, gk > 0], [RAGGED_GEMM, RAGGED_FUSED, GROUPED], SHARED)      # train.hip:541, 549, 562; 969-979
    kout = np.where(gk > 0, gk, K)                                                               # train.hip:539, 883, 943
    Kp = np.select([rag, gk > 0], [up64(kmax), 8], up64(K))                                      # train.hip:943 (569 for the shared set)
    hdt = np.where(unr, v["img_dt"], F16)                                                        # train.hip:951
    operand = (mode == SHARED) | (mode == RAGGED_GEMM)                                           # train.hip:556, 572 / 574 against 558, 565
    return status, mode, kout, Kp, hdt, operand.astype(int), (v["hb_n"] > 0).astype(int), refusal      # train.hip:579, 958


def compare(v):
    got, want = call_entry(v), parent_conditions(v)
    names = ("status", "mode", "kout", "Kp", "hdt", "dgrad operand", "head blocks", "refusal")
    for col, (name, w) in enumerate(zip(names, want)):
        bad = np.flatnonzero(got[:, col] != w)
        assert bad.size == 0, f"{name} differs in {bad.size} rows, first: " + str({k: int(a[bad[0]]) for k, a in v.items()})
    return got


def test_plan_equals_the_parent_conditions_over_the_full_product():
    v = product_rows()
    assert len(v["K"]) == 5 * 6 * 5 * 5 * 2 * 2 * 3 * 2 * 2
    got = compare(v)
    # not vacuous: every mode, both outcomes of the refusal, the three kinds of pitch and both row dtypes occur among the accepted rows
    ok = got[:, 0] == 0
    assert set(got[ok, 1].tolist()) == {SHARED, GROUPED, RAGGED_GEMM, RAGGED_FUSED} and set(got[:, 0].tolist()) == {0, ERR_UNSUPPORTED}
    assert {8, 64, 128, 192, 256} <= set(got[ok, 3].tolist()) and set(got[ok, 4].tolist()) == {F16, BF16}
    assert set(got[ok, 5].tolist()) == {0, 1} and set(got[ok, 6].tolist()) == {0, 1}
    assert set(got[:, 7].tolist()) == {NO_REFUSAL, HEAD_BLOCKS_REFUSED, RAGGED_LOGITS, GROUP_SIZE}


def one(**kw):
    conf = dict(group_k=0, ragged=0, kmax=0, K=5, hb_n=0, arch_option=0, unrounded=0, img_dt=BF16, out_c=128, logits=0, ragged_gemm=0)
    conf.update(kw)
    return compare({k: np.array([x]) for k, x in conf.items()})[0].tolist()


def test_named_configurations():
    assert one(K=150) == [0, SHARED, 150, 192, F16, 1, 0, 0]
    assert one(K=150, unrounded=1) == [0, SHARED, 150, 192, BF16, 1, 0, 0]
    assert one(K=6, group_k=3, logits=1) == [0, GROUPED, 3, 8, F16, 0, 0, 0]
    assert one(K=5, ragged=1, kmax=3) == [0, RAGGED_FUSED, 5, 64, F16, 0, 0, 0]
    assert one(K=300, ragged=1, kmax=65, ragged_gemm=1) == [0, RAGGED_GEMM, 300, 128, F16, 1, 0, 0]
    assert one(K=5, hb_n=2, arch_option=1, logits=1) == [0, SHARED, 5, 64, F16, 1, 1, 0]
    # refusals
    assert one(K=5, ragged=1, kmax=3, logits=1)[::7] == [ERR_UNSUPPORTED, RAGGED_LOGITS]
    assert one(K=18, group_k=9)[::7] == [ERR_UNSUPPORTED, GROUP_SIZE]
    assert one(K=6, group_k=3, out_c=100)[::7] == [ERR_UNSUPPORTED, GROUP_SIZE]
    assert one(K=6, group_k=3, hb_n=1, arch_option=2)[::7] == [ERR_UNSUPPORTED, HEAD_BLOCKS_REFUSED]
    # the head blocks are reported before the logits output and before the size of the group
    assert one(K=5, ragged=1, kmax=3, hb_n=1, arch_option=1, logits=1)[::7] == [ERR_UNSUPPORTED, HEAD_BLOCKS_REFUSED]
    assert one(K=18, group_k=9, hb_n=1, arch_option=1)[::7] == [ERR_UNSUPPORTED, HEAD_BLOCKS_REFUSED]


def test_entry_refusals():
    lib = _lib.load()
    row, out = (C.c_int32 * 11)(), (C.c_int32 * 8)()
    assert lib.lseg_op_train_head_plan(None, 1, out) == ERR_INVALID
    assert lib.lseg_op_train_head_plan(row, 1, None) == ERR_INVALID
    assert lib.lseg_op_train_head_plan(row, 0, out) == ERR_INVALID
