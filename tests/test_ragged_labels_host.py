"""Host-side checks of the ragged per-image label sets (lseg_set_text_groups / lseg_op_corr_argmax_ragged, csrc/corr_argmax.hip RAGGED):
the new entries in the header, the library and the ctypes table, and a CPU model of how the launcher deals the labels of every image to
label parts -- the parts are sized from the LARGEST list, an image with a shorter list owns fewer of them, and the kernel / merge pair
must see every label of every image in exactly one non-empty part made of whole panels."""
import ctypes as C
import os
import re

import pytest

from lseg_hip import _lib

_ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["lseg_set_text_groups", "lseg_op_corr_argmax_ragged", "lseg_op_corr_argmax_ragged_split"]


def _header_arity(name):
    src = open(os.path.join(_ROOT, "include", "lseg_hip.h")).read()
    m = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)\s*;", src)
    assert m, f"{name} is not declared in include/lseg_hip.h"
    return len([p for p in m.group(1).split(",") if p.strip()])


@pytest.mark.parametrize("name", NEW)
def test_new_entries_are_declared_bound_and_exported_with_matching_arity(name):
    assert name in _lib.SIGNATURES
    res, args = _lib.SIGNATURES[name]
    assert len(args) == _header_arity(name)
    assert hasattr(_lib.load(), name)
    assert _lib.load().lseg_abi_version() == 1             # additive: the ABI version stays


def test_the_ragged_op_is_the_conf_op_with_counts_and_offsets_instead_of_K():
    # (g, T, scale, [host_counts, d_offsets], 5 outputs, B, [K] H, W, C, ws, ws_bytes, stream)
    assert _header_arity("lseg_op_corr_argmax_ragged") == _header_arity("lseg_op_corr_argmax_conf") + 1


def _panel():
    out8 = (C.c_int * 8)()
    _lib.check(_lib.load().lseg_op_corr_argmax_geometry(out8))
    return out8[3]


def _split(counts, H, W, conf, ws_bytes, cus):
    out2 = (C.c_int * 2)()
    arr = (C.c_int32 * len(counts))(*counts)
    _lib.check(_lib.load().lseg_op_corr_argmax_ragged_split(arr, len(counts), H, W, conf, ws_bytes, cus, out2))
    return out2[0], out2[1]


COUNTS = [(1,), (48,), (47, 49), (1, 300), (1000, 2)]
# (H, W, compute units planned for): one tile per image on a whole chip, nine tiles, and a chip so small that splitting never pays
PLANS = [(6, 6, 256), (30, 30, 256), (9, 17, 64), (6, 6, 1)]


@pytest.mark.parametrize("conf", [0, 1])
@pytest.mark.parametrize("H,W,cus", PLANS)
@pytest.mark.parametrize("counts", COUNTS)
def test_every_label_of_every_image_falls_in_exactly_one_non_empty_part_of_whole_panels(counts, H, W, cus, conf):
    P = _panel()
    B, npix = len(counts), len(counts) * 16 * H * W
    for room in (0, 1, 2, 3, 8):                           # workspace for this many parts
        nsplit, per = _split(counts, H, W, conf, room * npix * (16 if conf else 6), cus)
        assert 1 <= nsplit <= max(1, room) and nsplit <= 8
        assert per % P == 0 and per >= P
        assert nsplit * per >= max(counts), "the largest list does not fit the parts"
        assert (nsplit - 1) * per < max(counts), "the last part is empty even for the largest list"
        for b in range(B):
            seen = [0] * counts[b]
            # the kernel: part s of image b streams [s * per, min((s + 1) * per, count)) and returns at once when that is empty;
            # the merge reads ceil(count / per) parts of the image (csrc/corr_argmax.hip ca_parts_of)
            parts = [(s * per, min((s + 1) * per, counts[b])) for s in range(nsplit) if s * per < counts[b]]
            assert len(parts) == min(nsplit, -(-counts[b] // per)) >= 1
            for i, (lo, hi) in enumerate(parts):
                assert hi > lo and lo % P == 0
                assert (hi - lo) % P == 0 or i == len(parts) - 1, "a part other than the image's last is not whole panels"
                for k in range(lo, hi):
                    seen[k] += 1
            assert seen == [1] * counts[b]
    # a whole chip and one tile per image: the long lists ARE split when there is room (the test above must not be vacuous)
    if cus == 256 and H == 6 and max(counts) > 2 * P:
        assert _split(counts, H, W, conf, 8 * npix * 16, cus)[0] > 1


def test_counts_outside_the_int16_labels_are_refused_on_the_host():
    lib = _lib.load()
    out2 = (C.c_int * 2)()
    for bad in ((0,), (3, 0), (-1, 5), (32768,), (5, 40000)):
        arr = (C.c_int32 * len(bad))(*bad)
        assert lib.lseg_op_corr_argmax_ragged_split(arr, len(bad), 6, 6, 1, 0, 256, out2) == -1        # LSEG_ERR_INVALID
    assert lib.lseg_op_corr_argmax_ragged_split(None, 1, 6, 6, 1, 0, 256, out2) == -1
    assert _split((32767,), 6, 6, 1, 0, 256) == (1, -(-32767 // _panel()) * _panel())
