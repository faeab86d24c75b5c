"""Host side of the windowed multi-scale evaluator (no device needed): the three C entries are declared, exported and bound with the
header's arity, their argument checks come before any HIP call, and the window partition BatchedMultiEval uses for a scale that does not
fit in max_stack is whole boxes, ascending, disjoint and covering."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from lseg_hip import _lib
from lseg_hip.evaluator import BatchedMultiEval, ModuleSurface, ScaleGeometry, plan_schedule, scale_geometry, window_partition

LSEG_ERR_INVALID = -1
assert _lib.STATUS[LSEG_ERR_INVALID] == "LSEG_ERR_INVALID"

ARITY = {"lseg_op_eval_accumulate_window": 15, "lseg_op_eval_accumulate_window_lowres": 15, "lseg_op_eval_finalize": 12}


def test_header_declares_and_binding_binds_the_window_entries(repo_root):
    hdr = open(os.path.join(repo_root, "include", "lseg_hip.h")).read()
    raw = C.CDLL(_lib.LIB_PATH)                        # the built library itself, not the binding's view of it
    lib = _lib.load()
    for name, arity in ARITY.items():
        m = re.search(r"^int\s+" + name + r"\s*\(([^;]*)\)\s*;", hdr, re.M)
        assert m, f"{name} is not declared in include/lseg_hip.h"
        assert len(m.group(1).split(",")) == arity, name
        assert hasattr(raw, name), name
        assert name in _lib.SIGNATURES, name
        res, args = _lib.SIGNATURES[name]
        assert res is C.c_int and len(args) == arity, name
        assert args[0] is C.c_void_p and args[1] is C.c_void_p and args[-1] is C.c_void_p and all(a is C.c_int for a in args[2:-1]), name
        assert getattr(lib, name).restype is C.c_int


# ---- the partition -------------------------------------------------------------------------------------------------------------------
# (h_grids, w_grids), max_stack, flip
PARTITIONS = [((1, 1), 2, True), ((4, 3), 4, True), ((4, 3), 4, False), ((4, 3), 5, True), ((4, 3), 5, False), ((4, 3), 24, True),
              ((4, 3), 24, False)]


@pytest.mark.parametrize("grid,max_stack,flip", PARTITIONS)
def test_window_partition_is_whole_boxes_ascending_disjoint_covering(grid, max_stack, flip):
    n = grid[0] * grid[1]
    twins = 2 if flip else 1
    wins = window_partition(n, max_stack, flip)
    # numpy model: how often each box of the grid is visited, and in which order
    visits = np.zeros(n, dtype=np.int64)
    order = []
    for first, nb in wins:
        assert isinstance(first, int) and isinstance(nb, int) and nb >= 1 and 0 <= first and first + nb <= n
        assert twins * nb <= max_stack, (first, nb)
        visits[first:first + nb] += 1
        order.extend(range(first, first + nb))
    assert (visits == 1).all()                          # disjoint and covering
    assert order == list(range(n))                      # ascending, across and within windows
    # no window could have been larger: all but the last are as full as max_stack allows
    per = max_stack // twins
    assert all(nb == per for _, nb in wins[:-1]) and len(wins) == -(-n // per)


def test_window_partition_with_an_odd_remainder():
    """max_stack 5 with flip: a box and its twin are never split, so windows hold 2 boxes = 4 crops and the fifth slot stays empty."""
    assert window_partition(12, 5, True) == [(0, 2), (2, 2), (4, 2), (6, 2), (8, 2), (10, 2)]
    assert window_partition(12, 5, False) == [(0, 5), (5, 5), (10, 2)]
    assert window_partition(12, 24, True) == [(0, 12)]
    assert window_partition(1, 2, True) == [(0, 1)]


def test_window_partition_refuses_a_max_stack_below_one_box_with_its_twin():
    with pytest.raises(ValueError):
        window_partition(12, 1, True)
    with pytest.raises(ValueError):
        window_partition(12, 0, False)
    assert window_partition(12, 1, False) == [(i, 1) for i in range(12)]


# ---- the geometry and the plan --------------------------------------------------------------------------------------------------------
SCALES = (0.5, 0.75, 1.0, 1.25, 1.5, 1.75)
# crop 480: (base, (h, w)) -> the plain tuples scale_geometry returned before it named its fields
WORKLOADS = {
    (520, (512, 683)): [(195, 260, 480, 480, 1, 1, 320), (292, 390, 480, 480, 1, 1, 320), (390, 520, 480, 520, 1, 2, 320),
                        (487, 650, 487, 650, 2, 2, 320), (585, 780, 585, 780, 2, 2, 320), (682, 910, 682, 910, 2, 3, 320)],
    (2048, (1024, 2048)): [(512, 1024, 512, 1024, 2, 3, 320), (768, 1536, 768, 1536, 2, 5, 320), (1024, 2048, 1024, 2048, 3, 6, 320),
                           (1280, 2560, 1280, 2560, 4, 8, 320), (1536, 3072, 1536, 3072, 5, 10, 320), (1792, 3584, 1792, 3584, 6, 11, 320)],
}


def _geometries(base, hw):
    return [scale_geometry(hw[0], hw[1], s, base, 480) for s in SCALES]


@pytest.mark.parametrize("base,hw", list(WORKLOADS))
def test_scale_geometry_is_the_plain_tuple_with_named_fields(base, hw):
    for g, want in zip(_geometries(base, hw), WORKLOADS[(base, hw)]):
        assert g == want and tuple(g) == want and len(g) == 7
        height, width, ph, pw, h_grids, w_grids, stride = g
        assert (height, width, ph, pw, h_grids, w_grids, stride) == want
        assert (g.height, g.width, g.ph, g.pw, g.h_grids, g.w_grids, g.stride) == want
        assert g[4] * g[5] == g.n_box == h_grids * w_grids


def test_plan_of_the_ade_shaped_image_is_one_stack():
    """crop 480 / base 520, 512x683, flip: 36 crops with their twins, one batch-36 forward (profiles/eval_lowres.txt)."""
    geo = _geometries(520, (512, 683))
    assert [2 * g.n_box for g in geo] == [2, 2, 4, 8, 8, 12]
    steps, largest = plan_schedule(geo, True, 48, 36)
    assert [(list(s.scales), s.windows) for s in steps] == [([0, 1, 2, 3, 4, 5], None)]
    assert largest == 36


def test_plan_of_the_base_2048_image_windows_the_three_large_scales():
    """crop 480 / base 2048, 1024x2048, flip, max_stack 48: scales 1.25, 1.5 and 1.75 in windows of 36 crops (profiles/eval_window.txt)."""
    geo = _geometries(2048, (1024, 2048))
    assert [2 * g.n_box for g in geo] == [12, 20, 36, 64, 100, 132]
    steps, largest = plan_schedule(geo, True, 48, 36)
    assert [(list(s.scales), s.windows) for s in steps] == [
        ([0, 1], None), ([2], None),
        ([3], [(0, 18), (18, 14)]), ([4], [(0, 18), (18, 18), (36, 14)]), ([5], [(0, 18), (18, 18), (36, 18), (54, 12)])]
    assert largest == 36


def _grids(*hw):
    return [ScaleGeometry(0, 0, 0, 0, hg, wg, 1) for hg, wg in hw]       # the plan reads the grid alone


# geometries, max_stack, max_batch, flip
PLANS = [(_geometries(2048, (1024, 2048)), 48, 36, True),                   # max_stack > max_batch
         (_geometries(2048, (1024, 2048)), 24, 36, True),                   # max_stack < max_batch
         (_geometries(2048, (1024, 2048)), 192, 36, True),                  # everything fits in one stack
         (_geometries(520, (512, 683)), 8, 8, False),
         (_grids((1, 1), (1, 2), (2, 3)), 4, 8, True),                      # tests/test_gpu_eval_window.py's image
         (_grids((1, 1), (4, 3), (1, 1)), 2, 36, True),                     # max_stack == twins: one box and its twin per window
         (_grids((1, 1), (4, 3), (1, 1)), 1, 36, False),
         (_grids((4, 3), (2, 2)), 5, 1, True),                              # max_batch holds no box with its twin: windows of max_stack
         (_grids((4, 3), (2, 2)), 5, 3, True)]


@pytest.mark.parametrize("geo,max_stack,max_batch,flip", PLANS)
def test_plan_properties(geo, max_stack, max_batch, flip):
    twins = 2 if flip else 1
    crops = [twins * g.n_box for g in geo]
    steps, largest = plan_schedule(geo, flip, max_stack, max_batch)
    assert [i for s in steps for i in s.scales] == list(range(len(geo)))      # every scale in exactly one step, in order
    per_fwd = min(max_stack, max_batch)
    window_cap = per_fwd if per_fwd >= twins else max_stack
    forwards = []
    for s in steps:
        if s.windows is None:
            assert all(crops[i] <= max_stack for i in s.scales)
            assert sum(crops[i] for i in s.scales) <= max_stack
            forwards.append(sum(crops[i] for i in s.scales))
        else:
            (i,) = s.scales
            assert crops[i] > max_stack
            assert s.windows == window_partition(geo[i].n_box, window_cap, flip)
            assert all(twins * nb <= window_cap for _, nb in s.windows)
            forwards.extend(twins * nb for _, nb in s.windows)
    assert largest == max(forwards)
    # greedy: a stack could not have taken the first scale of the next step
    for a, b in zip(steps, steps[1:]):
        if a.windows is None and b.windows is None:
            assert sum(crops[i] for i in a.scales) + crops[b.scales[0]] > max_stack


def test_max_stack_is_a_constructor_argument_and_the_attribute_still_overrides():
    import torch
    surf = ModuleSurface(torch.nn.Identity(), crop_size=64, base_size=72)
    ev = BatchedMultiEval(surf, 5)
    assert ev._max_stack is None and not hasattr(ev, "max_stack")          # None: the defaults (48 / 192 with lowres)
    ev = BatchedMultiEval(surf, 5, max_stack=6)
    assert ev._max_stack == 6
    ev.max_stack = 20                                   # the override that existed before the argument did
    assert ev.max_stack == 20
    del ev.max_stack
    assert ev._max_stack == 6


# ---- argument checks, before any HIP call ---------------------------------------------------------------------------------------------
def _geom(**kw):
    g = dict(K=2, height=12, width=16, ph=12, pw=16, crop=12, stride=8, hg=1, wg=2, flip=1, first=0, nb=2)
    g.update(kw)
    return g


def _window(lib, name, outs, summ, **kw):
    g = _geom(**kw)
    return getattr(lib, name)(outs, summ, g["K"], g["height"], g["width"], g["ph"], g["pw"], g["crop"], g["stride"], g["hg"], g["wg"], g["flip"],
                              g["first"], g["nb"], None)


def _finalize(lib, summ, out, **kw):
    g = _geom(**kw)
    return lib.lseg_op_eval_finalize(summ, out, g["K"], g["height"], g["width"], g["ph"], g["pw"], g["crop"], g["stride"], g["hg"], g["wg"], None)


@pytest.mark.parametrize("name", ["lseg_op_eval_accumulate_window", "lseg_op_eval_accumulate_window_lowres"])
def test_window_entries_reject_bad_arguments_before_touching_a_device(name):
    lib = _lib.load()
    # host buffers stand in for device memory: every call below must return from the argument checks, before any HIP call
    outs = (C.c_float * (4 * 2 * 12 * 12))()
    summ = (C.c_float * (2 * 12 * 16))()
    po, ps = C.cast(outs, C.c_void_p), C.cast(summ, C.c_void_p)
    assert _window(lib, name, None, ps) == LSEG_ERR_INVALID
    assert _window(lib, name, po, None) == LSEG_ERR_INVALID
    for nb in (0, -1):
        assert _window(lib, name, po, ps, nb=nb) == LSEG_ERR_INVALID, nb
    assert _window(lib, name, po, ps, first=1, nb=2) == LSEG_ERR_INVALID          # boxes [1, 3) of a 2-box grid
    assert _window(lib, name, po, ps, first=2, nb=1) == LSEG_ERR_INVALID
    assert _window(lib, name, po, ps, first=-1, nb=1) == LSEG_ERR_INVALID
    assert b"window" in lib.lseg_last_error(None)
    assert _window(lib, name, po, ps, wg=1, nb=1) == LSEG_ERR_INVALID             # one 12-wide box does not cover 16 columns
    assert _window(lib, name, po, ps, height=13) == LSEG_ERR_INVALID              # height > ph
    assert _window(lib, name, C.c_void_p(po.value + 2), ps) == LSEG_ERR_INVALID   # not a float address
    if name.endswith("lowres"):
        for crop in (13, 11, 3, 2, 0, -4):             # odd, or below 4
            assert _window(lib, name, po, ps, crop=crop) == LSEG_ERR_INVALID, crop
        assert b"crop" in lib.lseg_last_error(None)
    assert all(v == 0.0 for v in summ)


def _accumulate(lib, outs, out, **kw):
    g = _geom(**kw)
    return lib.lseg_op_eval_accumulate(outs, out, g["K"], g["height"], g["width"], g["ph"], g["pw"], g["crop"], g["stride"], g["hg"], g["wg"],
                                       g["flip"], None)


def test_accumulate_rejects_bad_arguments_before_touching_a_device():
    """The list of test_accumulate_lowres_rejects_bad_arguments_before_touching_a_device without the crop-parity cases.  Every call returns
    LSEG_ERR_INVALID (a missing device would be another status) and the message names the failed check."""
    lib = _lib.load()
    outs = (C.c_float * (4 * 2 * 12 * 12))()
    out = (C.c_float * (2 * 12 * 16))()
    po, pm = C.cast(outs, C.c_void_p), C.cast(out, C.c_void_p)
    assert _accumulate(lib, None, pm) == LSEG_ERR_INVALID
    assert _accumulate(lib, po, None) == LSEG_ERR_INVALID
    assert b"eval_accumulate: NULL" in lib.lseg_last_error(None)
    assert _accumulate(lib, po, pm, wg=1) == LSEG_ERR_INVALID                      # one 12-wide box does not cover 16 columns
    assert b"eval_accumulate: the boxes do not cover" in lib.lseg_last_error(None)
    assert _accumulate(lib, po, pm, height=13) == LSEG_ERR_INVALID                 # height > ph
    assert _accumulate(lib, C.c_void_p(po.value + 2), pm) == LSEG_ERR_INVALID      # not a float address
    assert b"aligned" in lib.lseg_last_error(None)
    assert all(v == 0.0 for v in out)


def test_accumulate_coverage_is_computed_in_64_bits():
    """Two boxes at stride INT_MAX with crop 1 reach row INT_MAX + 1 >= ph = 8: the coverage check passes, where (h_grids - 1) * stride +
    crop in int wraps negative and reports boxes that do not cover the map.  The call is then rejected by the NEXT check, the pointers'
    alignment, so nothing is launched."""
    lib = _lib.load()
    outs = (C.c_float * 16)()
    out = (C.c_float * (2 * 8 * 1))()
    po, pm = C.cast(outs, C.c_void_p), C.cast(out, C.c_void_p)
    big = dict(height=8, width=1, ph=8, pw=1, crop=1, stride=2 ** 31 - 1, hg=2, wg=1)
    assert _accumulate(lib, C.c_void_p(po.value + 2), pm, **big) == LSEG_ERR_INVALID
    msg = lib.lseg_last_error(None)
    assert b"cover" not in msg and b"aligned" in msg, msg
    assert _accumulate(lib, C.c_void_p(po.value + 2), pm, **dict(big, hg=1)) == LSEG_ERR_INVALID      # one box of crop 1 does not reach row 7
    assert b"cover" in lib.lseg_last_error(None)


def test_finalize_rejects_bad_arguments_before_touching_a_device():
    lib = _lib.load()
    summ = (C.c_float * (2 * 12 * 16))()
    ps = C.cast(summ, C.c_void_p)
    assert _finalize(lib, None, ps) == LSEG_ERR_INVALID
    assert _finalize(lib, ps, None) == LSEG_ERR_INVALID
    assert _finalize(lib, ps, ps, wg=1) == LSEG_ERR_INVALID
    assert _finalize(lib, ps, ps, K=0) == LSEG_ERR_INVALID
