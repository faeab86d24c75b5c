"""uint8 image input, the part that needs no GPU: the new symbols and their declared signatures, the arithmetic the uint8 first stages
must reproduce (pinned against torch's host kernels for all 256 byte values x 3 channels), and the argument checks that are decided
before a device is looked for."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

from lseg_hip import _lib

from input_u8_helpers import HALF, IMAGENET, normalize_table_numpy, to_tensor_normalize

_ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("lseg_set_input_u8", "lseg_op_patch_rows", "lseg_op_patch_rows_u8", "lseg_op_rn_stem_u8", "lseg_op_eval_make_crops_u8")


def F3(*v):
    return (C.c_float * 3)(*v)


def err(lib):
    return lib.lseg_last_error(None).decode()


def test_new_symbols_are_exported_and_declared():
    lib = _lib.load()
    header = open(os.path.join(_ROOT, "include", "lseg_hip.h")).read()
    for name in NEW:
        assert hasattr(lib, name), name
        res, args = _lib.SIGNATURES[name]
        assert res is C.c_int
        m = re.search(r"\bint " + name + r"\(([^;]*)\);", header)
        assert m, f"{name} is not declared in include/lseg_hip.h"
        assert len([a for a in m.group(1).split(",") if a.strip()]) == len(args), name       # one ctypes argument per declared parameter
    assert lib.lseg_abi_version() == 1                         # additive: the ABI version stays


@pytest.mark.parametrize("mean,std", [HALF, IMAGENET, ((0.1, 0.9, 0.333), (0.7, 1.0, 3.0))])
def test_three_fp32_operations_reproduce_totensor_normalize_bit_for_bit(mean, std):
    """Every byte value in every channel: float32 div, sub, div (what csrc/input_u8.hip's table holds) == ToTensor + Normalize on the host."""
    img = torch.arange(256, dtype=torch.uint8).view(1, 256, 1).expand(1, 256, 3).contiguous()      # [H=1, W=256, 3]
    ref = to_tensor_normalize(img, mean, std)                                                       # [3, 1, 256]
    tab = normalize_table_numpy(mean, std)
    assert ref.dtype == torch.float32 and tab.dtype == np.float32
    assert np.array_equal(ref.view(3, 256).numpy().view(np.uint32), tab.view(np.uint32))
    # the operations' order matters: one rounding less (a double detour) or a reciprocal multiply is NOT the same table
    recip = ((np.arange(256, dtype=np.float32)[None, :] * np.float32(1.0 / 255.0)) - np.asarray(mean, np.float32)[:, None]) / np.asarray(std, np.float32)[:, None]
    assert not np.array_equal(recip.astype(np.float32).view(np.uint32), tab.view(np.uint32))


def test_setter_refuses_bad_values_before_it_looks_at_the_handle():
    lib = _lib.load()
    ok = F3(0.5, 0.5, 0.5)
    for bad, word in ((F3(0.5, 0.0, 0.5), "std[1] is 0"), (F3(0.5, 0.5, float("inf")), "not finite"), (F3(float("nan"), 0.5, 0.5), "not finite")):
        assert lib.lseg_set_input_u8(None, 1, ok, bad) == -1 and word in err(lib), err(lib)          # LSEG_ERR_INVALID, by value
    assert lib.lseg_set_input_u8(None, 1, F3(0.5, float("inf"), 0.5), ok) == -1 and "not finite" in err(lib)
    assert lib.lseg_set_input_u8(None, 1, None, ok) == -1 and "NULL" in err(lib)
    assert lib.lseg_set_input_u8(None, 1, ok, ok) == -1 and "NULL handle" in err(lib)                # good values: the handle is next
    assert lib.lseg_set_input_u8(None, 0, None, None) == -1 and "NULL handle" in err(lib)            # switching off reads no values


def test_op_entries_check_their_arguments_without_a_device():
    lib = _lib.load()
    ok, zero = F3(0.5, 0.5, 0.5), F3(0.5, 0.5, 0.0)
    a = 1 << 12                                                # an aligned non-NULL address: no entry gets as far as reading it here
    bf = _lib.LSEG_BF16
    # patch rows
    assert lib.lseg_op_patch_rows_u8(a, a, 1, 32, 48, 16, bf, ok, zero, None) == -1 and "std[2] is 0" in err(lib)
    assert lib.lseg_op_patch_rows_u8(None, a, 1, 32, 48, 16, bf, ok, ok, None) == -1
    assert lib.lseg_op_patch_rows_u8(a, a, 1, 32, 40, 16, bf, ok, ok, None) == -1                    # W no multiple of P
    assert lib.lseg_op_patch_rows_u8(a, a, 1, 32, 40, 8, bf, ok, ok, None) == -5                     # P % 16: LSEG_ERR_UNSUPPORTED
    assert lib.lseg_op_patch_rows_u8(a + 4, a, 1, 32, 48, 16, bf, ok, ok, None) == -1 and "aligned" in err(lib)
    assert lib.lseg_op_patch_rows_u8(a, a, 1, 32, 48, 16, _lib.LSEG_F32, ok, ok, None) == -1
    assert lib.lseg_op_patch_rows(a, a, 1, 32, 44, 4, bf, None) == -5                                # the float pack: P % 8
    assert lib.lseg_op_patch_rows(a, a, 1, 32, 48, 16, _lib.LSEG_F32, None) == -1
    # stem
    assert lib.lseg_op_rn_stem_u8(a, a, a, a, 1, 64, 63, bf, ok, ok, None) == -1                     # odd width
    assert lib.lseg_op_rn_stem_u8(a, a, None, a, 1, 64, 64, bf, ok, ok, None) == -1
    assert lib.lseg_op_rn_stem_u8(a, a, a, a, 1, 64, 64, bf, zero, zero, None) == -1
    # evaluator crops
    assert lib.lseg_op_eval_make_crops_u8(a, a, 40, 56, 30, 42, 32, 21, 1, 2, 1, ok, ok, zero, None) == -1
    assert lib.lseg_op_eval_make_crops_u8(a, a, 40, 56, 30, 42, 32, 21, 1, 0, 1, ok, ok, ok, None) == -1 and "geometry" in err(lib)
    assert lib.lseg_op_eval_make_crops_u8(a, None, 40, 56, 30, 42, 32, 21, 1, 2, 1, ok, ok, ok, None) == -1
    if not torch.cuda.is_available():                          # valid arguments, no device: LSEG_ERR_NO_DEVICE, never a fallback
        assert lib.lseg_op_patch_rows_u8(a, a, 1, 32, 48, 16, bf, ok, ok, None) == -2, err(lib)      # (with a device this would launch on a
        assert lib.lseg_op_rn_stem_u8(a, a, a, a, 1, 64, 64, bf, ok, ok, None) == -2, err(lib)       # made-up address: not called there)
        assert lib.lseg_op_eval_make_crops_u8(a, a, 40, 56, 30, 42, 32, 21, 1, 2, 1, ok, ok, ok, None) == -2, err(lib)


def test_python_surface_checks_that_need_no_engine():
    from lseg_hip.engine import HipEngine, image_dims
    assert image_dims(torch.zeros((2, 3, 8, 6))) == (2, 8, 6)
    assert image_dims(torch.zeros((2, 8, 6, 3), dtype=torch.uint8)) == (2, 8, 6)

    class Stub:                                                 # the two format refusals of _check_input need no device
        input_u8, device, img_h, img_w = None, torch.device("cpu"), 8, 6     # (None: the default format is float32 NCHW)
        _group, _groups, _K = 0, None, 1
    s, check = Stub(), HipEngine._check_input
    with pytest.raises(_lib.LSegError) as e:
        check(s, torch.zeros((1, 8, 6, 3), dtype=torch.uint8))
    assert e.value.code == -1 and "set_input_u8" in str(e.value)
    s.input_u8 = HALF
    with pytest.raises(_lib.LSegError) as e:
        check(s, torch.zeros((1, 3, 8, 6)))
    assert e.value.code == -1 and "set_input_u8(False)" in str(e.value)
    with pytest.raises(_lib.LSegError) as e:
        check(s, torch.zeros((1, 3, 8, 6), dtype=torch.uint8))       # NCHW uint8: the wrong layout
    assert e.value.code == -1 and "HWC" in str(e.value)
    assert check(s, torch.zeros((1, 8, 6, 3), dtype=torch.uint8)).shape == (1, 8, 6, 3)
    odd = torch.arange(8 + 8 * 6 * 3, dtype=torch.uint8)[8:].view(1, 8, 6, 3)       # 8 bytes in: contiguous, not 16-byte aligned
    assert odd.data_ptr() % 16 == 8 and odd.is_contiguous()
    got = check(s, odd)
    assert got.data_ptr() % 16 == 0 and torch.equal(got, odd)                       # handed on as an aligned copy


def test_evaluator_refuses_a_host_uint8_image_by_name():
    from lseg_hip.evaluator import BatchedMultiEval, ModuleSurface
    ev = BatchedMultiEval(ModuleSurface(torch.nn.Identity(), crop_size=32, base_size=56), 5, scales=(1.0,))
    with pytest.raises(ValueError, match="move it to the GPU"):
        ev.forward(torch.zeros((40, 56, 3), dtype=torch.uint8))
