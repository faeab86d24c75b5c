"""Host-side checks of the large-K mask path (csrc/corr_argmax.hip, lseg_forward_labels): the exported entries, and a CPU index model
of the kernel's tile -> footprint mapping, in the style of tests/test_kernel_index_models.py.

The x2 o x2 align_corners footprint is NOT tile-aligned: a tile is a band of CA_LB = 28 rows / columns of the (2h, 2w) "mid" map and
owns the output pixels whose upper-left mid tap lies in the band; the mid pixels those read (band + 1) read base pixels in turn.  The
model restates the kernel's float32 formulas (src_tap of common.h, ca_first_out / ca_end_out and the origin of corr_argmax_kernel) and
pins what the kernel relies on: every output pixel is owned by exactly one tile, all four mid taps and all base taps behind them lie
inside that tile's 29 x 29 mid / 16 x 16 base footprint, and the owned pixels fit the thread layout (64 columns = lanes, 4 x 15 rows)."""
import ctypes as C

import numpy as np
import pytest

from lseg_hip import _lib

f32 = np.float32


@pytest.fixture(scope="module")
def geo():
    """the constants the kernel was compiled with (lseg_op_corr_argmax_geometry): the model follows the kernel, not a copy of its numbers:
    (CA_LB, CA_MT, CA_BT, CA_P, CA_PITCH, CA_LC, CA_ROWS, CA_LDS)"""
    out = (C.c_int * 8)()
    _lib.check(_lib.load().lseg_op_corr_argmax_geometry(out))
    return tuple(out)


def test_library_exports_the_label_entries():
    lib = C.CDLL(_lib.LIB_PATH)
    for name in ("lseg_forward_labels", "lseg_op_corr_argmax", "lseg_op_corr_argmax_geometry"):
        assert hasattr(lib, name), name
    assert _lib.load().lseg_abi_version() == 1


def _ratio(n_in, n_out):
    return f32(f32(n_in - 1) / f32(n_out - 1))


def _src_tap(r, i, n):                                    # common.h src_tap(): product rounded to float32 before the floor
    s = f32(r * f32(i))
    i0 = int(s)
    return i0, i0 + (1 if i0 < n - 1 else 0)


def _first_out(r, a):                                     # corr_argmax.hip ca_first_out()
    o = int(np.ceil(f32(f32(a) / r)))
    while o > 0 and int(f32(r * f32(o - 1))) >= a:
        o -= 1
    while int(f32(r * f32(o))) < a:
        o += 1
    return o


def _end_out(r, first, a_end, n_out):                     # ca_end_out()
    o = first
    while o < n_out and int(f32(r * f32(o))) < a_end:
        o += 1
    return o


def _axis_tiles(n, CA_LB):
    """per tile of one axis with n base pixels: (mid origin a, last mid index read, base origin, owned outputs [first, end))"""
    n_mid, n_out = 2 * n, 4 * n
    r1, r2 = _ratio(n, n_mid), _ratio(n_mid, n_out)
    out = []
    for a in range(0, n_mid, CA_LB):
        b_mid = min(a + CA_LB, n_mid - 1)
        lo = int(f32(r1 * f32(a)))
        first = _first_out(r2, a)
        out.append((a, b_mid, lo, first, _end_out(r2, first, a + CA_LB, n_out)))
    return out, r1, r2


@pytest.mark.parametrize("h,w", [(15, 15), (30, 30), (120, 120), (6, 6), (2, 2), (7, 30), (30, 17), (13, 120), (16, 14), (29, 57), (128, 96)])
def test_every_output_pixel_has_one_owner_and_its_footprint_inside_the_tile(geo, h, w):
    CA_LB, CA_MT, CA_BT, _, _, _, CA_ROWS, _ = geo
    for n, max_out in ((h, 4 * CA_ROWS), (w, 64)):        # the mapping is separable: rows (4 waves x 15 rows) and columns (64 lanes)
        tiles, r1, r2 = _axis_tiles(n, CA_LB)
        n_mid, n_out = 2 * n, 4 * n
        owner = np.zeros(n_out, dtype=np.int64)
        for a, b_mid, lo, first, end in tiles:
            assert 0 < end - first <= max_out, (n, a, first, end)
            owner[first:end] += 1
            per = (end - first + 3) // 4
            assert per <= CA_ROWS
            for o in range(first, end):
                m0, m1 = _src_tap(r2, o, n_mid)
                assert a <= m0 < a + CA_LB and m0 <= m1 <= b_mid, (n, a, o, m0, m1)      # both mid taps inside the band + 1
                assert m1 - a < CA_MT
                for m in (m0, m1):
                    b0, b1 = _src_tap(r1, m, n)
                    assert lo <= b0 <= b1 <= min(lo + CA_BT - 1, n - 1), (n, a, o, m, b0, b1, lo)   # base taps inside the 16-pixel fragment
            # what stage 1 stages -- mid indices a .. b_mid -- stays inside the fragment too (the launcher's ca_tiles_fit)
            for m in range(a, b_mid + 1):
                b0, b1 = _src_tap(r1, m, n)
                assert lo <= b0 and b1 - lo < CA_BT
        assert (owner == 1).all(), (n, np.flatnonzero(owner != 1)[:8])


def test_panel_and_staging_fit_the_lds(geo):
    CA_LB, CA_MT, CA_BT, P, pitch, lc, _, CA_LDS = geo
    assert CA_MT == CA_LB + 1 and CA_BT == 16 and pitch >= 512 * 2 and pitch % 16 == 0
    t = P * pitch
    rs = P * (CA_BT * CA_BT + 4) * 4
    lr = lc * ((CA_MT * CA_MT + 3) // 4 * 4) * 4
    assert P % 16 == 0 and t + rs + lr + 64 * 16 == CA_LDS <= 160 * 1024
    # the 16 labels of one accumulator store (lane c = label, 16 bytes each) start in different banks
    assert len({((c * (CA_BT * CA_BT + 4)) % 64) // 4 for c in range(16)}) == 16
