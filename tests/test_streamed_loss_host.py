"""Host-side checks of the streamed loss (no GPU): the symbols are exported and bound, the routes of LSegNet.forward_metrics exclude each
other, and the numpy model of the valid-pixel rule and of the reduction's partial layout (tests/streamed_loss_helpers.py) agrees with
the constants the library reports (lseg_op_corr_argmax_loss_plan / _ws_bytes)."""
import ctypes as C
import inspect

import numpy as np
import pytest

from lseg_hip import _lib
from streamed_loss_helpers import nll_model, owner_of, reduce_model, valid_mask

THREADS, MIN_PIXELS, MAX_GROUPS = 256, 4096, 1024          # csrc/corr_argmax.hip CL_*


@pytest.fixture(scope="module")
def lib():
    return _lib.load()


def test_symbols_are_exported_and_bound(lib):
    for name, nargs in (("lseg_op_corr_argmax_loss", 20), ("lseg_forward_labels_loss", 12), ("lseg_op_corr_argmax_loss_ws_bytes", 7),
                        ("lseg_op_corr_argmax_loss_plan", 4)):
        fn = getattr(lib, name)
        assert name in _lib.SIGNATURES and len(_lib.SIGNATURES[name][1]) == nargs
        assert fn.argtypes is not None and len(fn.argtypes) == nargs and fn.restype is _lib.SIGNATURES[name][0]
    from lseg_hip.engine import HipEngine
    sig = inspect.signature(HipEngine.forward_labels_loss)
    assert list(sig.parameters)[1:] == ["x", "target", "ignore_index", "plane"]
    assert sig.parameters["ignore_index"].default == -1 and sig.parameters["plane"].default is False


def test_streamed_and_panel_exclude_each_other_and_the_default_is_unchanged():
    from lseg_hip.config import get_config
    from modules.models.lseg_net import LSegNet
    sig = inspect.signature(LSegNet.forward_metrics)
    assert sig.parameters["streamed"].default is False and sig.parameters["panel"].default is None
    cfg = get_config("tiny16")
    net = LSegNet(labels=["a", "b", "c"], backbone="tiny16", features=cfg.features, arch_option=0, block_depth=0, activation="lrelu")
    with pytest.raises(ValueError, match="streamed"):
        net.forward_metrics(None, None, streamed=True, panel=16)          # refused before anything is looked at


def test_the_reduction_plan_is_the_documented_layout(lib):
    out4 = (C.c_int64 * 4)()
    for Bn, H, W in ((1, 2, 2), (2, 6, 6), (2, 15, 15), (3, 6, 6), (1, 16, 16), (1, 16, 17), (8, 120, 120), (36, 120, 120), (1, 1000, 1000)):
        _lib.check(lib.lseg_op_corr_argmax_loss_plan(Bn, H, W, out4))
        n = Bn * 16 * H * W
        chunk, groups, nbytes = reduce_model(n, THREADS, MIN_PIXELS, MAX_GROUPS)
        assert list(out4) == [THREADS, chunk, groups, nbytes], (Bn, H, W, list(out4))
        assert chunk % THREADS == 0 and 1 <= groups <= MAX_GROUPS and (groups - 1) * chunk < n <= groups * chunk    # no empty workgroup
        # the workspace: offsets, partials and temporary planes, each rounded up to 256 bytes, then 14 bytes per pixel and part
        up = lambda v: -(-v // 256) * 256                                                                           # noqa: E731
        assert lib.lseg_op_corr_argmax_loss_ws_bytes(Bn, H, W, 0, 0, 0, 0) == 0
        assert lib.lseg_op_corr_argmax_loss_ws_bytes(Bn, H, W, 1, 1, 2, 0) == up(4 * (Bn + 1)) + up(nbytes) + 2 * up(4 * n)
        assert lib.lseg_op_corr_argmax_loss_ws_bytes(Bn, H, W, 0, 1, 0, 8) == up(nbytes) + 8 * n * 14
    assert lib.lseg_op_corr_argmax_loss_plan(1, 6, 6, None) == -1 and lib.lseg_op_corr_argmax_loss_plan(0, 6, 6, out4) == -1
    # every pixel has exactly one owner, and lane t of workgroup j takes j * chunk + t + threads * m
    n = 2 * 16 * 15 * 15
    chunk, groups, _ = reduce_model(n, THREADS, MIN_PIXELS, MAX_GROUPS)
    j, lane, step = owner_of(n, chunk, THREADS)
    assert np.array_equal(j * chunk + lane + THREADS * step, np.arange(n)) and j.max() == groups - 1 and lane.max() == THREADS - 1


def test_valid_rule_and_the_ordered_sum():
    t = np.array([[[-1, 0, 4, 5, 255, -3]], [[2, 3, 1, 0, 7, 255]]])
    assert valid_mask(t, 255, 5).tolist() == [[[False, True, True, False, False, False]], [[True, True, True, True, False, False]]]
    assert valid_mask(t, -1, 5)[0, 0, 0] == False and valid_mask(t, 4, 5)[0, 0, 2] == False       # noqa: E712  (ignore_index wins over a label id)
    assert valid_mask(t, 255, [5, 3]).tolist() == [[[False, True, True, False, False, False]], [[True, False, True, True, False, False]]]
    # the sum in the kernel's order is a reordering of the plain float64 sum of non-negative terms: inside n * 2^-52 relative
    rng = np.random.default_rng(0)
    n = 2 * 16 * 15 * 15
    lse = (rng.random(n) * 20).astype(np.float32)
    tl = lse - (rng.random(n) * 9).astype(np.float32)
    valid = rng.random(n) < 0.8
    chunk, _, _ = reduce_model(n, THREADS, MIN_PIXELS, MAX_GROUPS)
    s = nll_model(lse, tl, valid, chunk, THREADS)
    ref = (lse.astype(np.float64) - tl.astype(np.float64))[valid].sum()
    assert abs(s - ref) <= valid.sum() * 2.0 ** -52 * ref and s > 0
