"""Host-side self-check of tests/conv_helpers.py and of the launcher's choices for the conv family: a plain fp32 emulation of every operation
(ascending k) passes the comparisons tests/test_gpu_conv_family.py uses, wrong variants fail them -- through the same functions --, the
launcher's plan names the epilogue, the tile and the work items per workgroup every GPU case was written for (at 256 and at 64 compute
units), the engine's split-K plan tiles K, the entries refuse malformed cases without a device, and the input conditions of every case
hold on the reference alone.  Needs no GPU.

One variant the issue names cannot be told apart by any test: "out_relu taken before the rounding".  round_T(max(v, 0)) and the stored
round_T(v) with its negative half cleared are the same bits for every finite v (rounding is monotone and keeps the sign).  Its place is
taken by the ReLU copy taken before the skips are added; "keeping -0" is tested as stated."""
import ctypes as C

import pytest
import torch

import conv_helpers as H
from lseg_hip import _lib

ERR_INVALID, ERR_UNSUPPORTED = -1, -5


@pytest.fixture(scope="module")
def lib():
    return _lib.load()


def rejected(what, name, fn):
    with pytest.raises(AssertionError) as e:
        fn()
    print(f"wrong-variant {what} [{name}]: {str(e.value).splitlines()[0]}")


# ---- the emulations pass ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", H.FORWARD, ids=H.ids(H.FORWARD))
def test_forward_emulation_passes_and_input_conditions_hold(c):
    d = H.fdata(c)
    H.check_forward(c, d, H.emulate_forward(c, d), who="host.")
    cond = H.CONDITIONS[c["name"]]
    if c["relu"]:
        assert 0.25 <= cond["neg_pre"] <= 0.75, f"{c['name']}: {cond['neg_pre']:.2f} of the pre-activations are negative"
    if c["relu_in"]:
        assert cond["neg_in"] >= 0.25, f"{c['name']}: {cond['neg_in']:.2f} of the inputs are negative"
    if c["out_relu"]:
        assert cond["neg_stored"] >= 1, f"{c['name']}: no stored value is negative"


@pytest.mark.parametrize("c", H.SPLIT, ids=H.ids(H.SPLIT))
def test_split_emulation_passes(c):
    d = H.fdata(c)
    H.check_split(c, d, H.emulate_split(c, d), who="host.")


@pytest.mark.parametrize("c", H.REDUCE, ids=H.ids(H.REDUCE))
def test_reduce_emulation_passes_and_input_conditions_hold(c):
    d = H.rdata(c)
    H.check_reduce(c, d, H.emulate_reduce(c, d), who="host.")
    cond = H.CONDITIONS[c["name"]]
    if c["relu"]:
        assert 0.25 <= cond["neg_pre"] <= 0.75
    if c["out_relu"]:
        assert cond["neg_stored"] >= 1


@pytest.mark.parametrize("c", H.WGRAD, ids=H.ids(H.WGRAD))
def test_wgrad_emulation_passes_and_wrong_variants_fail(c):
    d = H.wdata(c)
    H.check_wgrad(c, d, H.emulate_wgrad(c, d), c["slabs"], who="host.")
    if c["relu_x"]:
        assert (d["x"].float() < 0).float().mean() >= 0.25
    rejected("tap shift with the wrong sign", c["name"], lambda: H.check_wgrad(c, d, H.emulate_wgrad(c, d, "shift-sign"), c["slabs"], who="host.wrong."))
    if c["relu_x"]:
        rejected("relu_x ignored", c["name"], lambda: H.check_wgrad(c, d, H.emulate_wgrad(c, d, "relu_x-ignored"), c["slabs"], who="host.wrong."))
    if (c["B"] * (c["H"] + 2) * (c["W"] + 2)) % 64:
        rejected("k_valid tail rows read as data", c["name"], lambda: H.check_wgrad(c, d, H.emulate_wgrad(c, d, "tail-as-data"), c["slabs"], who="host.wrong."))


@pytest.mark.parametrize("c", H.WLIN, ids=H.ids(H.WLIN))
def test_linear_wgrad_emulation_passes_and_wrong_variants_fail(c):
    d = H.ldata(c)
    H.check_wlin(c, d, H.emulate_wlin(c, d), who="host.")
    if c["M"] % 64:
        rejected("k_valid tail rows read as data", c["name"], lambda: H.check_wlin(c, d, H.emulate_wlin(c, d, "tail-as-data"), who="host.wrong."))
    if c["acc"]:
        rejected("accumulate ignored", c["name"], lambda: H.check_wlin(c, d, H.emulate_wlin(c, d, "no-accumulate"), who="host.wrong."))


@pytest.mark.parametrize("c", H.PACK3 + H.PACK1, ids=H.ids(H.PACK3 + H.PACK1))
def test_packer_emulation_passes_and_pad_channel_is_caught(c):
    d = H.pdata(c)
    H.check_pack(c, d, H.emulate_pack(c, d), who="host.")
    if c.get("Cip", c["Ci"]) > c["Ci"]:
        rejected("a pad channel left non-zero", c["name"], lambda: H.check_pack(c, d, H.emulate_pack(c, d, "pad-channel"), who="host.wrong."))


def test_dgrad_pack_reference_is_the_transposed_convs_weight():
    """conv_transpose2d(dy, w) == conv2d(dy, flip(w).transpose(0, 1), padding=2 - pad): the reference permutation against autograd."""
    c = H.DGRAD_PACK[0]
    d = H.dgrad_pack_data(c)
    w = d["w4"].double()[:8, :16]
    dy = torch.randn(1, 8, 5, 5, dtype=torch.float64, generator=torch.Generator().manual_seed(3))
    x = torch.zeros(1, 16, 5, 5, dtype=torch.float64, requires_grad=True)
    (gx,) = torch.autograd.grad((torch.nn.functional.conv2d(x, w, padding=1) * dy).sum(), x)
    wd = H.dgrad_pack_ref(dict(w4=w)).reshape(16, 3, 3, 8).permute(0, 3, 1, 2)          # back to [Ci, Co, 3, 3]
    assert torch.allclose(torch.nn.functional.conv2d(dy, wd, padding=1), gx, atol=1e-12)


# ---- the wrong variants fail every case they apply to ----------------------------------------------------------------------------------------------
def _fw(wrong, cs, what):
    assert cs
    for c in cs:
        d = H.fdata(c)
        rejected(what, c["name"], lambda: H.check_forward(c, d, H.emulate_forward(c, d, wrong), who="host.wrong."))


def test_ky_kx_transposed_fails():
    _fw("kykx", [c for c in H.FORWARD if c["k"] == 3], "ky / kx transposed")


def test_stride2_origin_off_by_one_fails():
    _fw("stride-origin", [c for c in H.FORWARD if c["s"] == 2], "stride-2 origin off by one")


def test_tile_row_with_the_previous_images_base_fails():
    def straddles(c):
        e, hw = H.TILE_EDGE[c["exp"][1]], H.out_hw(c)[0] * H.out_hw(c)[1]
        return any((m // e) * e // hw != m // hw for m in range(c["B"] * hw))

    cs = [c for c in H.FORWARD if straddles(c)]
    assert len(cs) > len(H.FORWARD) // 2
    _fw("image-base-of-tile", cs, "a tile row of image b + 1 computed with image b's base")


def test_zeros_written_into_the_output_border_fail():
    _fw("zero-border", H.FORWARD, "zeros written into the output border")
    for c in H.REDUCE:
        d = H.rdata(c)
        rejected("zeros written into the output border", c["name"], lambda: H.check_reduce(c, d, H.emulate_reduce(c, d, "zero-border"), who="host.wrong."))


def test_input_border_read_as_zero_fails():
    _fw("border-as-zero", [c for c in H.FORWARD if c["k"] == 3], "the input border read as zero")


def test_relu_on_the_wrong_side_of_the_skips_fails():
    _fw("relu-side", [c for c in H.FORWARD if c["relu"] and c["nres"]], "ReLU on the wrong side of the skips")
    for c in [c for c in H.REDUCE if c["relu"] and c["nres"]]:
        d = H.rdata(c)
        rejected("ReLU on the wrong side of the skips", c["name"], lambda: H.check_reduce(c, d, H.emulate_reduce(c, d, "relu-side"), who="host.wrong."))


def test_res2_dropped_fails():
    _fw("drop-res2", [c for c in H.FORWARD if c["nres"] == 2], "res2 dropped")
    for c in [c for c in H.REDUCE if c["nres"] == 2]:
        d = H.rdata(c)
        rejected("res2 dropped", c["name"], lambda: H.check_reduce(c, d, H.emulate_reduce(c, d, "drop-res2"), who="host.wrong."))


def test_wrong_relu_copies_fail():
    _fw("outrelu-keeps-minus-zero", [c for c in H.FORWARD if c["out_relu"]], "out_relu keeps -0")
    _fw("outrelu-before-skips", [c for c in H.FORWARD if c["out_relu"] and c["nres"]], "out_relu taken before the skips")
    for c in [c for c in H.REDUCE if c["out_relu"]]:
        d = H.rdata(c)
        rejected("out_relu keeps -0", c["name"], lambda: H.check_reduce(c, d, H.emulate_reduce(c, d, "outrelu-keeps-minus-zero"), who="host.wrong."))


def test_split_ranges_dropped_or_started_early_fail():
    for c in H.SPLIT:
        d = H.fdata(c)
        rejected("one split range dropped", c["name"], lambda: H.check_split(c, d, H.emulate_split(c, d, "drop-range"), who="host.wrong."))
        rejected("a split range started a step early", c["name"], lambda: H.check_split(c, d, H.emulate_split(c, d, "range-early"), who="host.wrong."))
    for c in [c for c in H.REDUCE if c["name"].startswith("reduce.plain")]:
        d = H.rdata(c)
        rejected("the last slab dropped", c["name"], lambda: H.check_reduce(c, d, H.emulate_reduce(c, d, "drop-range"), who="host.wrong."))


# ---- the launcher's plan and the refusals, without a device ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("cus", [256, 64])
def test_plan_names_what_every_case_was_written_for(lib, cus):
    for c in H.FORWARD + H.SPLIT:
        H.assert_plan(lib, c, H.struct_of(c), cus)


def test_split_cases_begin_mid_tap_and_end_short():
    """Cin = 128: a tap is two K-steps.  Odd split_steps: some range begins in the second half of a tap; 4 x 5 of 18: a short last range."""
    assert any(c["steps"] % 2 == 1 and c["steps"] > 1 for c in H.SPLIT) and any(c["steps"] == 1 for c in H.SPLIT)
    assert any(c["nsplit"] * c["steps"] > 18 for c in H.SPLIT)
    for c in H.SPLIT:
        assert c["Cin"] == 128 and (c["nsplit"] - 1) * c["steps"] < 18 <= c["nsplit"] * c["steps"]


def test_malformed_conv_cases_are_refused_without_a_device(lib):
    base = next(c for c in H.EPILOGUE if c["name"] == "epi.outrelu.co128.t2.bf16")
    out4 = (C.c_int * 4)()
    for over, want in ((dict(ksize=2), ERR_INVALID), (dict(stride=3), ERR_INVALID), (dict(tile=3), ERR_INVALID), (dict(max_grid=12), ERR_INVALID),
                       (dict(dtype=_lib.LSEG_F32), ERR_INVALID), (dict(inp=None), ERR_INVALID), (dict(relu_after_res=1), ERR_INVALID),
                       (dict(residual2=H.FAKE), ERR_INVALID), (dict(Cin=96), ERR_UNSUPPORTED), (dict(nsplit=2, split_steps=5), ERR_INVALID),
                       (dict(bias=None), ERR_UNSUPPORTED), (dict(Cout=64), ERR_UNSUPPORTED)):          # out_relu off the specialised epilogue
        g = H.struct_of(base)
        for k, v in over.items():
            setattr(g, k, v)
        assert lib.lseg_op_conv_ex_plan(C.byref(g), 256, C.byref(out4)) == want, over
        assert lib.lseg_op_conv_ex(C.byref(g), None) == want, over
    c = next(c for c in H.SPLIT if c["name"] == "split.t2.4x5.bf16")
    for over in (dict(split_steps=4), dict(nsplit=5), dict(c_split_stride=16), dict(relu_out=1), dict(bias=H.FAKE)):
        g = H.struct_of(c)
        for k, v in over.items():
            setattr(g, k, v)
        assert lib.lseg_op_conv_ex(C.byref(g), None) == ERR_INVALID, over


def test_reduce_wgrad_and_packer_entries_refuse_before_a_device(lib):
    F = H.FAKE
    assert lib.lseg_op_conv_reduce_pad(F, 2, 4096, F, None, None, F, None, 1, 2, 2, 12, 0, 0, _lib.LSEG_BF16, None) == ERR_UNSUPPORTED      # C % 8
    assert lib.lseg_op_conv_reduce_pad(None, 2, 4096, F, None, None, F, None, 1, 2, 2, 8, 0, 0, _lib.LSEG_BF16, None) == ERR_INVALID
    assert lib.lseg_op_conv_reduce_pad(F, 2, 4096, F, None, None, None, None, 1, 2, 2, 8, 0, 0, _lib.LSEG_BF16, None) == ERR_INVALID
    assert lib.lseg_op_conv_reduce_pad(F, 0, 4096, F, None, None, F, None, 1, 2, 2, 8, 0, 0, _lib.LSEG_BF16, None) == ERR_INVALID
    assert lib.lseg_op_conv_reduce_pad(F, 2, 16, F, None, None, F, None, 1, 2, 2, 8, 0, 0, _lib.LSEG_BF16, None) == ERR_INVALID              # slabs overlap
    for part, res, res2, out, out_relu in ((F + 4, F, F, F, F), (F, F + 2, F, F, F), (F, F, F + 8, F, F), (F, F, F, F + 2, F), (F, F, F, F, F + 6)):
        assert lib.lseg_op_conv_reduce_pad(part, 2, 4096, F, res, res2, out, out_relu, 1, 2, 2, 8, 0, 0, _lib.LSEG_BF16, None) == ERR_INVALID   # 16-byte alignment
    assert lib.lseg_op_conv_wgrad(F, F, F, 0, 1, 4, 4, 64, 64, F, 1 << 24, _lib.LSEG_BF16, None) == ERR_UNSUPPORTED                        # Cin % 128
    assert lib.lseg_op_conv_wgrad(F, F, F, 0, 1, 4, 4, 128, 64, F, 64 * 9 * 128 - 1, _lib.LSEG_BF16, None) == ERR_UNSUPPORTED              # workspace
    assert lib.lseg_op_wgrad_kmajor(F, 48, F, 200, 37, 40, 192, F, 0, F, 1 << 24, _lib.LSEG_BF16, None) == ERR_UNSUPPORTED                 # cols % 128
    assert lib.lseg_op_wgrad_kmajor(F, 48, F, 136, 37, 40, 128, F, 0, F, 40 * 128 - 1, _lib.LSEG_BF16, None) == ERR_UNSUPPORTED
    assert lib.lseg_op_wgrad_kmajor(F, 32, F, 136, 37, 40, 128, F, 0, F, 1 << 24, _lib.LSEG_BF16, None) == ERR_INVALID                     # ldy < rows_out
    assert lib.lseg_op_conv_dgrad_pack(None, F, 64, 64, None) == ERR_INVALID
    assert lib.lseg_op_pack_conv3x3(F, None, None, None, None, 1e-5, None, F, None, 8, 16, 8, _lib.LSEG_BF16, None) == ERR_INVALID         # Cip < Ci
    assert lib.lseg_op_pack_conv3x3(F, F, None, F, F, 1e-5, None, F, None, 8, 8, 8, _lib.LSEG_BF16, None) == ERR_INVALID
    assert lib.lseg_op_pack_conv1x1(F, None, None, None, None, 1e-5, F, None, 8, 8, _lib.LSEG_BF16, None) == ERR_INVALID


# ---- the engine's split-K plan ---------------------------------------------------------------------------------------------------------------------------
def _engine_convs():
    """(label, M, N, K) of the convs Engine::conv3x3 runs: the DPT head at 480 x 480 (features 256; layerN_rn from the ViT-L/16 reassemble
    widths 256, 512, 1024, 1024; the residual units 256 -> 256) on the four pyramid levels 120, 60, 30, 15, and the 3x3 / 1x1 convs of the
    ResNet-101 stages (widths 64 .. 512, expansion 4) at 120 .. 15."""
    out = []
    for B in (1, 4, 36):
        for lvl, (hw, cin) in enumerate(zip((120, 60, 30, 15), (256, 512, 1024, 1024))):
            out.append((f"B{B}.layer{lvl + 1}_rn", B * hw * hw, 256, 9 * cin))
            out.append((f"B{B}.rcu{lvl + 1}", B * hw * hw, 256, 9 * 256))
        for st, (hw, wd) in enumerate(zip((120, 60, 30, 15), (64, 128, 256, 512))):
            out.append((f"B{B}.rn{st + 1}.conv2", B * hw * hw, wd, 9 * wd))
            out.append((f"B{B}.rn{st + 1}.conv3", B * hw * hw, 4 * wd, wd))
            out.append((f"B{B}.rn{st + 1}.conv1", B * hw * hw, wd, 4 * wd))
    return out


def _inline_plan(M, N, K, ws_floats):
    """The arithmetic Engine::conv3x3 carried inline before it was lifted into conv_splitk_plan, transcribed.  A pin against later edits of
    either side, not evidence about the move itself; the properties asserted beside it are the test."""
    nk = K // 64
    tiles = ((M + 63) // 64) * (N // 64)
    ns = min(512 // tiles, nk // 8, 8)
    while ns > 1 and ns * M * N > ws_floats:
        ns -= 1
    if ns >= 2:
        steps = (nk + ns - 1) // ns
        ns = (nk + steps - 1) // steps
    return (ns, (nk + ns - 1) // ns) if ns >= 2 else (1, nk)


@pytest.mark.parametrize("ws_floats", [16384 * 1024, 1 << 20])
def test_conv_splitk_plan_tiles_K_and_fits_the_workspace(lib, ws_floats):
    seen = set()
    for label, M, N, K in _engine_convs():
        ns, steps = C.c_int(), C.c_int()
        assert lib.lseg_op_conv_splitk_plan(M, N, K, ws_floats, C.byref(ns), C.byref(steps)) == 0
        ns, steps, nk = ns.value, steps.value, K // 64
        assert (ns, steps) == _inline_plan(M, N, K, ws_floats), label
        tiles = -(-M // 64) * (N // 64)
        assert 1 <= ns <= 8, label
        assert ns * steps >= nk and (ns - 1) * steps < nk, f"{label}: {ns} x {steps} does not tile {nk} steps"          # every range non-empty
        if ns > 1:
            assert ns * M * N <= ws_floats and steps >= 8 and ns * tiles <= 512 + tiles, label
        if tiles > 256:
            assert ns == 1, f"{label}: {tiles} tiles already fill the chip, split {ns}"
        seen.add(ns)
        print(f"conv-splitk-plan ws={ws_floats} {label}: M={M} N={N} K={K} -> ns={ns} steps={steps}")
    assert 1 in seen and max(seen) > 1
    assert lib.lseg_op_conv_splitk_plan(64, 96, 576, ws_floats, C.byref(C.c_int()), C.byref(C.c_int())) == ERR_INVALID
