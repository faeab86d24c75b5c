"""The route table of Engine::forward (csrc/forward_route.h, through lseg_op_forward_route: host only, no device) against a transcription
of the conditions the forward had before they were gathered there -- csrc/engine.hip at commit 6cd5509, cited by line -- over the full
cross product of requests, label-set sizes, configurations and environment switches.  Requests the forward refuses before a launch
are compared on the status, the others on the tail, the source of the label planes and the three schedule flags."""
import ctypes as C

import numpy as np
import pytest

from lseg_hip import _lib

ERR_INVALID, ERR_UNSUPPORTED = -1, -5
HELD, STREAM_RAGGED, STREAM_SHARED, X4_LOGITS, X2_LOW_OUT, PLANES, FEAT_COMMUTED, FEAT_ROWNORM, FEAT_HEAD1 = range(9)
NO_PLANES, FUSED, GROUPED, GENERIC = range(4)

# corr.hip:261  corr_planes_supported: C == 512 and K x CORR_PITCH (1040 B) <= 160 KiB of LDS
K_FIT = 160 * 1024 // 1040
assert (K_FIT, K_FIT * 1040 <= 160 * 1024 < (K_FIT + 1) * 1040) == (157, True)
KS = [1, K_FIT, K_FIT + 1, 256, 257, 32767, 32768]

# columns of a request row, in the entry's order; `wanted` is split into its bits here
BITS = ["logits", "argmax", "label", "score", "low", "runner_up", "lse", "held", "loss"]       # bit 9, the loss's target, follows `loss`
CONF = ["group_k", "ragged", "arch_option", "out_c", "lw0", "headc", "corr_full", "corr_generic", "no_4x"]
CONF_VALUES = [(0, 3), (0, 1), (0, 1), (128, 512), (6, 7), (0, 1), (0, 1), (0, 1), (0, 1)]


def product_rows(K, debug, strict):
    """every request x configuration for one K, debug, strict: a dict of int64 columns, 2^9 x 2^9 = 262144 rows"""
    axes = [(0, 1)] * len(BITS) + CONF_VALUES
    grid = np.array(np.meshgrid(*axes, indexing="ij")).reshape(len(axes), -1).astype(np.int64)
    v = dict(zip(BITS + CONF, grid))
    n = grid.shape[1]
    v.update(target=v["loss"].copy(), K=np.full(n, K), debug=np.full(n, int(debug)), strict=np.full(n, int(strict)))
    return v


def call_entry(v):
    n = len(v["K"])
    wanted = sum(v[b] << i for i, b in enumerate(BITS)) + (v["target"] << 9)
    cols = [wanted, v["K"], v["group_k"], v["ragged"], v["arch_option"], v["out_c"], v["lw0"], v["debug"], v["strict"], v["headc"],
            v["corr_full"], v["corr_generic"], v["no_4x"]]
    rows = np.ascontiguousarray(np.stack(cols, axis=1).astype(np.int32))
    out = np.full((n, 6), -99, np.int32)
    assert _lib.load().lseg_op_forward_route(rows.ctypes.data_as(C.c_void_p), n, out.ctypes.data_as(C.c_void_p)) == 0
    return out


def parent_conditions(v):
    """engine.hip at 6cd5509, Engine::forward (1047-1318) with check_ragged (694-709) and check_held (726-738): (status, tail, planes,
    commuted, corr_low, corr_fused) per row.  First true condition wins, in the order of the code."""
    b = {k: a.astype(bool) for k, a in v.items() if k in BITS + ["target", "ragged", "headc", "corr_full", "corr_generic", "no_4x", "debug", "strict"]}
    K, gk, arch, out_c, lw0 = v["K"], v["group_k"], v["arch_option"], v["out_c"], v["lw0"]
    conf_any = b["runner_up"] | b["lse"]
    commuted = ~b["debug"] & ~b["strict"] & b["headc"]                                           # 1166 (704, 730: the same expression)
    labels_only = b["label"] & ~b["logits"] & ~b["argmax"] & ~b["low"]                           # 1061, the argument of check_ragged
    status = np.select([
        conf_any & ~b["label"],                                                                  # 1051
        b["loss"] & (~b["label"] | ~b["target"] | b["runner_up"] | b["logits"] | b["argmax"] | b["low"] | b["held"]),        # 1052
        b["held"] & ((gk > 0) | b["ragged"]),                                                    # 1058 -> 729
        b["held"] & (~commuted | b["corr_full"] | (lw0 % 2 != 0) | (arch != 0)),                 # 1058 -> 733
        b["score"] & ~b["label"],                                                                # 1059
        b["label"] & ~b["ragged"] & (np.where(gk > 0, gk, K) > 32767),                           # 1060
        b["ragged"] & ~labels_only,                                                              # 1061 -> 701
        b["ragged"] & (~commuted | b["corr_full"] | (lw0 % 2 != 0) | b["corr_generic"] | (arch != 0) | (out_c != 512)),        # 1061 -> 705
    ], [ERR_INVALID, ERR_INVALID, ERR_UNSUPPORTED, ERR_UNSUPPORTED, ERR_INVALID, ERR_UNSUPPORTED, ERR_UNSUPPORTED, ERR_UNSUPPORTED], 0)
    corr_low = commuted & ~b["corr_full"] & (lw0 % 2 == 0)                                       # 1179
    planes_ok = (out_c == 512) & (K >= 1) & (K * 1040 <= 160 * 1024)                             # corr.hip:261
    argmax_ok = (out_c == 512) & (K >= 1) & (K <= 32767)                                         # corr_argmax.hip:616
    corr_fused = corr_low & ~b["held"] & ~b["corr_generic"] & (gk == 0) & ~b["ragged"] & planes_ok      # 1187 (inside `if (corr_low)`, 1180)
    streamed = b["label"] & ~b["logits"] & ~b["argmax"] & ~b["corr_generic"] & (gk == 0) & (arch == 0) & argmax_ok      # 1225
    x4 = b["logits"] & ~b["argmax"] & (arch == 0) & ~b["no_4x"]                                  # 1248
    x2 = b["low"] & ~b["logits"] & ~b["argmax"] & ~b["label"] & (arch == 0)                      # 1256
    tail = np.select([
        corr_low & b["held"],                                                                    # 1201
        corr_low & b["ragged"],                                                                  # 1216
        corr_low & streamed,                                                                     # 1225
        corr_low & x4, corr_low & x2, corr_low,                                                  # 1248, 1256, 1262
        commuted,                                                                                # 1263
        (out_c == 512) & ~b["debug"] & ~b["strict"],                                             # 1268
    ], [HELD, STREAM_RAGGED, STREAM_SHARED, X4_LOGITS, X2_LOW_OUT, PLANES, FEAT_COMMUTED, FEAT_ROWNORM], FEAT_HEAD1)      # 1274
    planes = np.where(tail < X4_LOGITS, NO_PLANES, np.where(tail > PLANES, NO_PLANES,
                      np.select([corr_fused, gk > 0], [FUSED, GROUPED], GENERIC)))               # 1233, 1234, 1239
    return status, tail, planes, commuted.astype(int), corr_low.astype(int), corr_fused.astype(int)


def compare(v):
    got = call_entry(v)
    status, *route = parent_conditions(v)
    assert np.array_equal(got[:, 0], status), f"status differs in {int((got[:, 0] != status).sum())} rows"
    ok = status == 0
    for col, (name, want) in enumerate(zip(("tail", "planes", "commuted", "corr_low", "corr_fused"), route), 1):
        bad = np.flatnonzero(ok & (got[:, col] != want))
        assert bad.size == 0, f"{name} differs in {bad.size} accepted rows, first: " + str({k: int(a[bad[0]]) for k, a in v.items()})
    return got, ok


@pytest.mark.parametrize("strict", [False, True])
@pytest.mark.parametrize("debug", [False, True])
@pytest.mark.parametrize("K", KS)
def test_route_equals_the_parent_conditions_over_the_full_product(K, debug, strict):
    got, ok = compare(product_rows(K, debug, strict))
    assert ok.any() and (~ok).any()


def test_every_tail_and_every_refusal_is_reached():
    """the comparison above is not vacuous: over the product every tail, every source of the planes and both refusal codes occur"""
    tails, planes, codes = set(), set(), set()
    for K in (K_FIT, K_FIT + 1):
        for debug in (False, True):
            v = product_rows(K, debug, False)
            got = call_entry(v)
            ok = got[:, 0] == 0
            tails |= set(got[ok, 1].tolist())
            planes |= set(got[ok, 2].tolist())
            codes |= set(got[:, 0].tolist())
    assert tails == set(range(9)) and planes == set(range(4)) and codes == {0, ERR_INVALID, ERR_UNSUPPORTED}


def one(K, wanted, **kw):
    conf = dict(group_k=0, ragged=0, arch_option=0, out_c=512, lw0=120, headc=1, corr_full=0, corr_generic=0, no_4x=0, debug=0, strict=0)
    conf.update(kw)
    v = {k: np.array([int(k in wanted)]) for k in BITS + ["target"]}
    v.update({k: np.array([x]) for k, x in conf.items()}, K=np.array([K]))
    got, _ = compare(v)
    return got[0].tolist()


def test_named_requests():
    """the table read for a few requests of the C entries (ViT-L/16 at 480 x 480: out_c 512, quarter-resolution width 120)"""
    # lseg_forward_lowres at K = 200, arch_option 0: pixel_gram + one GEMM for the planes, then the x2 upsample into the caller's buffer
    assert one(200, ["low"]) == [0, X2_LOW_OUT, GENERIC, 1, 1, 0]
    assert one(150, ["low"]) == [0, X2_LOW_OUT, FUSED, 1, 1, 1]
    assert one(150, ["logits"]) == [0, X4_LOGITS, FUSED, 1, 1, 1]
    assert one(150, ["logits"], no_4x=1) == [0, PLANES, FUSED, 1, 1, 1]
    assert one(150, ["logits", "argmax"]) == [0, PLANES, FUSED, 1, 1, 1]
    assert one(150, ["label", "score"]) == [0, STREAM_SHARED, NO_PLANES, 1, 1, 1]          # the gram still comes from corr_planes
    assert one(300, ["label", "lse", "loss", "target"]) == [0, STREAM_SHARED, NO_PLANES, 1, 1, 0]
    assert one(300, ["label"], arch_option=1) == [0, PLANES, GENERIC, 1, 1, 0]
    assert one(300, ["label"], ragged=1) == [0, STREAM_RAGGED, NO_PLANES, 1, 1, 0]
    assert one(6, ["logits"], group_k=3) == [0, X4_LOGITS, GROUPED, 1, 1, 0]
    assert one(5, ["held"]) == [0, HELD, NO_PLANES, 1, 1, 0]
    assert one(5, ["logits"], headc=0) == [0, FEAT_ROWNORM, NO_PLANES, 0, 0, 0]
    assert one(5, ["logits"], debug=1) == [0, FEAT_HEAD1, NO_PLANES, 0, 0, 0]                 # the debug taps read the fp32 feature map
    assert one(5, ["logits"], out_c=128, strict=1) == [0, FEAT_HEAD1, NO_PLANES, 0, 0, 0]
    assert one(5, ["logits"], corr_full=1) == [0, FEAT_COMMUTED, NO_PLANES, 1, 0, 0]
    assert one(5, ["logits"], lw0=7) == [0, FEAT_COMMUTED, NO_PLANES, 1, 0, 0]
    # refusals
    assert one(5, ["label", "loss"])[0] == ERR_INVALID                                       # a loss without its target
    assert one(5, ["score"])[0] == ERR_INVALID
    assert one(32768, ["label"])[0] == ERR_UNSUPPORTED
    assert one(32768, ["label"], ragged=1)[0] == 0                                           # the lists are bounded one by one
    assert one(5, ["logits"], ragged=1)[0] == ERR_UNSUPPORTED
    assert one(5, ["held"], debug=1)[0] == ERR_UNSUPPORTED


def test_entry_refusals():
    lib = _lib.load()
    row, out = (C.c_int32 * 13)(), (C.c_int32 * 6)()
    assert lib.lseg_op_forward_route(None, 1, out) == ERR_INVALID
    assert lib.lseg_op_forward_route(row, 1, None) == ERR_INVALID
    assert lib.lseg_op_forward_route(row, 0, out) == ERR_INVALID
