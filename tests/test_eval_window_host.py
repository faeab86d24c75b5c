"""Host side of the windowed multi-scale evaluator (no device needed): the three C entries are declared, exported and bound with the
header's arity, their argument checks come before any HIP call, and the window partition BatchedMultiEval uses for a scale that does not
fit in max_stack is whole boxes, ascending, disjoint and covering."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from lseg_hip import _lib
from lseg_hip.evaluator import BatchedMultiEval, ModuleSurface, window_partition

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


def test_finalize_rejects_bad_arguments_before_touching_a_device():
    lib = _lib.load()
    summ = (C.c_float * (2 * 12 * 16))()
    ps = C.cast(summ, C.c_void_p)
    assert _finalize(lib, None, ps) == LSEG_ERR_INVALID
    assert _finalize(lib, ps, None) == LSEG_ERR_INVALID
    assert _finalize(lib, ps, ps, wg=1) == LSEG_ERR_INVALID
    assert _finalize(lib, ps, ps, K=0) == LSEG_ERR_INVALID
