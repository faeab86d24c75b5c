"""Host side of the low-resolution multi-scale evaluator path (no device needed): the two C entries exist and are declared, the op's
argument checks come before any HIP call, and BatchedMultiEval(lowres=True) refuses a module that cannot give low-resolution logits."""
import ctypes as C

import pytest
import torch

from lseg_hip import _lib
from lseg_hip.evaluator import BatchedMultiEval, ModuleSurface

LSEG_ERR_INVALID = -1
assert _lib.STATUS[LSEG_ERR_INVALID] == "LSEG_ERR_INVALID"


def test_library_exports_and_binding_declares_the_lowres_entries():
    raw = C.CDLL(_lib.LIB_PATH)                        # the built library itself, not the binding's view of it
    for name in ("lseg_forward_lowres", "lseg_op_eval_accumulate_lowres"):
        assert hasattr(raw, name), name
        assert name in _lib.SIGNATURES, name
    assert len(_lib.SIGNATURES["lseg_forward_lowres"][1]) == 5
    assert len(_lib.SIGNATURES["lseg_op_eval_accumulate_lowres"][1]) == len(_lib.SIGNATURES["lseg_op_eval_accumulate"][1]) == 13
    lib = _lib.load()
    assert lib.lseg_op_eval_accumulate_lowres.restype is C.c_int


def _call(lib, low, out, crop, K=2, height=12, width=16, ph=12, pw=16, stride=8, hg=1, wg=2, flip=1):
    return lib.lseg_op_eval_accumulate_lowres(low, out, K, height, width, ph, pw, crop, stride, hg, wg, flip, None)


def test_accumulate_lowres_rejects_bad_arguments_before_touching_a_device():
    lib = _lib.load()
    # host buffers stand in for device memory: every call below must return from the argument checks, before any HIP call
    low = (C.c_float * (4 * 2 * 6 * 6))()
    out = (C.c_float * (2 * 12 * 16))()
    pl, po = C.cast(low, C.c_void_p), C.cast(out, C.c_void_p)
    assert _call(lib, None, po, 12) == LSEG_ERR_INVALID
    assert _call(lib, pl, None, 12) == LSEG_ERR_INVALID
    for crop in (13, 11, 3, 2, 0, -4):                 # odd, or below 4
        assert _call(lib, pl, po, crop) == LSEG_ERR_INVALID, crop
    assert b"crop" in lib.lseg_last_error(None)
    assert _call(lib, pl, po, 12, wg=1) == LSEG_ERR_INVALID            # one 12-wide box does not cover 16 columns
    assert _call(lib, pl, po, 12, height=13) == LSEG_ERR_INVALID       # height > ph
    assert _call(lib, C.c_void_p(pl.value + 2), po, 12) == LSEG_ERR_INVALID      # not a float address


class _NoLowres(torch.nn.Module):
    crop_size, base_size = 64, 72
    mean, std = [0.5] * 3, [0.5] * 3
    _up_kwargs = {"mode": "bilinear", "align_corners": True}

    def evaluate(self, x, target=None):
        raise AssertionError("must not be called")

    def evaluate_random(self, x, labelset, target=None):
        raise AssertionError("must not be called")


def test_lowres_evaluator_refuses_a_module_without_the_lowres_methods():
    BatchedMultiEval(_NoLowres(), 5)                                    # the default path asks for nothing new
    with pytest.raises((AttributeError, ValueError), match="evaluate_lowres"):
        BatchedMultiEval(_NoLowres(), 5, lowres=True)

    class _Half(_NoLowres):
        def evaluate_lowres(self, x):
            raise AssertionError("must not be called")

    with pytest.raises((AttributeError, ValueError), match="evaluate_random_lowres"):
        BatchedMultiEval(_Half(), 5, lowres=True)


def test_module_surfaces_offer_the_lowres_pair():
    from modules.lsegmentation_module import LSegmentationModule
    from modules.models.lseg_net import LSegNet
    for cls in (ModuleSurface, LSegmentationModule):
        assert callable(getattr(cls, "evaluate_lowres")) and callable(getattr(cls, "evaluate_random_lowres")), cls
    assert callable(getattr(LSegNet, "forward_lowres"))
    ev = BatchedMultiEval(ModuleSurface(torch.nn.Identity(), crop_size=64, base_size=72), 5, lowres=True)
    assert ev.lowres and not BatchedMultiEval(ModuleSurface(torch.nn.Identity()), 5).lowres
