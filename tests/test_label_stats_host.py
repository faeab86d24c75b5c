"""Host-side checks of the label statistics (csrc/label_stats.hip, lseg_hip.metrics): the numpy references the GPU tests compare against
tell the right rules from wrong ones on named cases; lseg_op_label_stats_plan on both sides of the LDS budget; every refusal of the
three ops that needs no launch; and the argument checks of the Python wrappers, which raise before anything is loaded."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

from label_stats_helpers import (emu_up2, fold_planes, fold_targets, nll_bound, partition_of, random_case, ref_label_stats, ref_nll,
                                 ref_panel_state)
from lseg_hip import _lib

_ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ERR_INVALID, ERR_UNSUPPORTED = -1, -5
LDS_BINS = 48 * 1024 // 12                                     # the budget csrc/label_stats.hip states: 3 x bins x 4 bytes <= 48 KiB


# ---- the count reference ------------------------------------------------------------------------------------------------------------------
def test_count_reference_on_a_hand_made_case():
    """2 x 3 pixels, K = 3, ignore_index 255: counted by hand"""
    lab = np.array([[[0, 1, 2], [2, 2, 0]]], np.int16)
    tgt = np.array([[[0, 2, -1], [2, 255, 7]]], np.int64)
    counts, flags = ref_label_stats(lab, tgt, 3, 255)
    #          correct labeled | inter      | pred (pixels 0, 1, 3, 5) | lab
    assert counts.tolist() == [2, 4, 1, 0, 1, 2, 1, 1, 1, 0, 2]
    assert flags.tolist() == [1, 0]                             # the 7


def test_count_reference_equals_seg_stats_rule_without_ignore_index():
    """metrics.py's rule on target + 1 / predict + 1 (what seg_stats_kernel implements), restated here, for targets without ignore_index"""
    lab, tgt = random_case(2, 6, 10, [7, 7], 3, ignore_index=-1)
    counts, _ = ref_label_stats(lab, tgt, 7, -1)
    l1, t1 = lab.astype(np.int64) + 1, tgt + 1
    labeled = (t1 > 0).sum()
    correct = ((l1 == t1) & (t1 > 0)).sum()
    p = l1 * (t1 > 0)
    inter = p * (p == t1)
    hist = lambda a: np.histogram(a, bins=7, range=(1, 7))[0]       # noqa: E731
    assert counts[0] == correct and counts[1] == labeled
    assert np.array_equal(counts[2:9], hist(inter)) and np.array_equal(counts[9:16], hist(p)) and np.array_equal(counts[16:23], hist(t1))


@pytest.mark.parametrize("variant,case", [("union_for_pred", "shared"), ("ignored_as_labeled", "shared"), ("map_pred_only", "mapped")])
def test_count_reference_rejects_wrong_variants(variant, case):
    if case == "shared":
        lab, tgt = random_case(2, 7, 13, [7, 7], 5)
        kw = dict(K=7, ignore_index=255)
    else:
        lab, tgt = random_case(2, 7, 13, [3, 5], 5)
        kw = dict(ignore_index=255, group_sizes=[3, 5], class_map=[4, 0, 2, 2, 1, 0, 3, 4], nclass=5)
    right = ref_label_stats(lab, tgt, **kw)[0]
    wrong = ref_label_stats(lab, tgt, variant=variant, **kw)[0]
    assert not np.array_equal(right, wrong), variant


def test_ragged_and_mapped_references_add_up():
    """ragged counts = the per-image shared-set counts laid side by side; a class map adds the bins of equal ids"""
    sizes = [1, 9, 2]
    lab, tgt = random_case(3, 6, 10, sizes, 11)
    ragged, rf = ref_label_stats(lab, tgt, ignore_index=255, group_sizes=sizes)
    n = sum(sizes)
    want, wf, off = np.zeros(2 + 3 * n, np.int64), np.zeros(2, np.int64), 0
    for b, k in enumerate(sizes):
        c, f = ref_label_stats(lab[b:b + 1], tgt[b:b + 1], k, 255)
        want[:2] += c[:2]
        wf += f
        for a in range(3):
            want[2 + a * n + off:2 + a * n + off + k] = c[2 + a * k:2 + (a + 1) * k]
        off += k
    assert np.array_equal(ragged, want) and np.array_equal(rf, wf)
    ident = list(range(n))                                      # the identity map over all list entries = the ragged layout
    assert np.array_equal(ref_label_stats(lab, tgt, ignore_index=255, group_sizes=sizes, class_map=ident, nclass=n)[0], ragged)
    cmap = [0, 1, 2, 3, 1, 2, 3, 0, 1, 2, 0, 3]                 # duplicates inside a list (image 1) and across lists
    mapped, _ = ref_label_stats(lab, tgt, ignore_index=255, group_sizes=sizes, class_map=cmap, nclass=4)
    for a in (1, 2):                                            # pred and lab are linear in the bins; inter gains the merged duplicates
        for c in range(4):
            assert mapped[2 + a * 4 + c] == sum(ragged[2 + a * n + i] for i in range(n) if cmap[i] == c)
    assert mapped[1] == ragged[1] and mapped[0] >= ragged[0]
    bad = list(cmap)
    bad[5] = 9                                                  # an id outside [0, nclass): that entry's pixels reach no bin, nothing else moves
    skipped, _ = ref_label_stats(lab, tgt, ignore_index=255, group_sizes=sizes, class_map=bad, nclass=4)
    assert skipped[1] == mapped[1] and skipped[2 + 4:2 + 8].sum() == mapped[2 + 4:2 + 8].sum() - ragged[2 + n + 5]


# ---- the panel state reference --------------------------------------------------------------------------------------------------------------
def _state_case(K=7, part=(5, 2)):
    low = fold_planes(2, K, 3, 5, "rand", 4, list(part))
    up = emu_up2(low)
    return up, fold_targets(2, K, 6, 10, list(part), 4)


def test_state_reference_is_the_argmax_the_gather_and_the_logsumexp():
    up, tgt = _state_case()
    label, best, s, tl = ref_panel_state(up, tgt, [5, 2])
    assert np.array_equal(label, up.argmax(axis=1).astype(np.int16))            # numpy's arg-max is the first maximum
    assert np.array_equal(best, up.max(axis=1).astype(np.float64))
    ties = (up == up.max(axis=1, keepdims=True)).sum(axis=1)
    assert (ties >= 2).any()                                                    # the planted ties are there
    valid = tgt >= 0
    gathered = np.take_along_axis(up.astype(np.float64), np.clip(tgt, 0, 6)[:, None], axis=1)[:, 0]
    assert np.array_equal(tl[valid], gathered[valid]) and np.isnan(tl[~valid]).all()
    nsum, ncount, m, px, v = ref_nll(up, tgt)
    assert np.abs((best + np.log(s) - tl)[v] - px[v]).max() <= 1e-12 and ncount == int(valid.sum())
    for part in ([1] * 7, [7], [3, 3, 1]):                                      # every partition: the same state
        l2, b2, s2, t2 = ref_panel_state(up, tgt, part)
        assert np.array_equal(l2, label) and np.array_equal(b2, best) and np.array_equal(t2[valid], tl[valid])
        assert np.abs(s2 - s).max() <= 1e-12


@pytest.mark.parametrize("variant", ["ge", "wrong_panel"])
def test_state_reference_rejects_wrong_variants(variant):
    up, tgt = _state_case()
    right = ref_panel_state(up, tgt, [5, 2])
    wrong = ref_panel_state(up, tgt, [5, 2], variant=variant)
    if variant == "ge":
        assert not np.array_equal(right[0], wrong[0])                           # the LAST maximum wins on the planted ties
    else:
        valid = tgt >= 0
        assert not np.array_equal(right[3][valid], wrong[3][valid])             # the target's logit read one panel too far


def test_nll_bound_is_small_against_the_loss_and_grows_with_k():
    up, tgt = _state_case()
    nsum, ncount, m, px, v = ref_nll(up, tgt)
    b7 = nll_bound(7, m, px, v)
    assert 0 < b7 < 1e-4 * abs(nsum)
    assert nll_bound(37, m, px, v) > b7


def test_emulated_upsample_interpolates_and_keeps_corners():
    low = fold_planes(1, 2, 4, 4, "rand", 1, [2])
    up = emu_up2(low)
    assert up.shape == (1, 2, 8, 8) and up.dtype == np.float32
    assert np.array_equal(up[..., 0, 0], low[..., 0, 0]) and np.abs(up[..., -1, -1] - low[..., -1, -1]).max() <= 1e-6
    assert up.min() >= low.min() - 1e-6 and up.max() <= low.max() + 1e-6
    assert np.array_equal(emu_up2(np.full((1, 1, 3, 5), 0.625, np.float32)), np.full((1, 1, 6, 10), 0.625, np.float32))


# ---- the plan ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bins,route,per_wg", [(1, 0, 1), (150, 0, 150), (LDS_BINS, 0, LDS_BINS), (LDS_BINS + 1, 1, 0), (32767, 1, 0),
                                               (100000, 1, 0)])
def test_plan_on_both_sides_of_the_lds_budget(bins, route, per_wg):
    lib = _lib.load()
    out = (C.c_int * 2)()
    assert lib.lseg_op_label_stats_plan(bins, out) == 0
    assert list(out) == [route, per_wg]
    assert 3 * out[1] * 4 <= 48 * 1024


def test_plan_refusals():
    lib = _lib.load()
    out = (C.c_int * 2)()
    assert lib.lseg_op_label_stats_plan(0, out) == ERR_INVALID
    assert lib.lseg_op_label_stats_plan(5, None) == ERR_INVALID


# ---- refusals: before any launch, so they need no device --------------------------------------------------------------------------------------
def _buf(n=64):
    b = (C.c_double * n)()
    return C.cast(b, C.c_void_p), b


def test_label_stats_refusals():
    lib = _lib.load()
    p, keep = _buf()
    ok = dict(label=p, target=p, B=1, H=2, W=2, K=3, ignore=-1, offsets=None, cmap=None, nclass=0, counts=p, flags=p)

    def call(**kw):
        a = dict(ok, **kw)
        return lib.lseg_op_label_stats(a["label"], a["target"], a["B"], a["H"], a["W"], a["K"], a["ignore"], a["offsets"], a["cmap"], a["nclass"],
                                       a["counts"], a["flags"], 0, None)
    for name in ("label", "target", "counts", "flags"):
        assert call(**{name: None}) == ERR_INVALID, name
    for name in ("B", "H", "W", "K"):
        assert call(**{name: 0}) == ERR_INVALID, name
    assert call(offsets=p, cmap=p, nclass=0) == ERR_INVALID
    assert call(cmap=p, nclass=4) == ERR_INVALID                                # a map without offsets
    assert call(K=32768) == ERR_UNSUPPORTED
    assert call(offsets=p, K=40000) == ERR_UNSUPPORTED                          # a count above 32767
    assert b"32767" in lib.lseg_last_error(None)


def test_fold_and_finish_refusals():
    lib = _lib.load()
    p, keep = _buf()

    def fold(low=p, B=1, rows=2, row0=0, h=2, w=2, target=p, label=p, best=p, s=p, tl=p):
        return lib.lseg_op_stats_fold_lowres(low, B, rows, row0, h, w, target, label, best, s, tl, 1, None)
    for name in ("low", "target", "label", "best", "s", "tl"):
        assert fold(**{name: None}) == ERR_INVALID, name
    for kw in (dict(B=0), dict(rows=0), dict(row0=-1), dict(h=1), dict(w=0)):
        assert fold(**kw) == ERR_INVALID, kw
    assert fold(row0=32766, rows=2) == ERR_UNSUPPORTED

    def finish(label=p, best=p, s=p, tl=p, target=p, B=1, H=4, W=4, K=3, counts=p, nll=p, flags=p, ws=p):
        return lib.lseg_op_stats_finish(label, best, s, tl, target, B, H, W, K, -1, counts, nll, flags, ws, 512, None)
    for name in ("label", "best", "s", "tl", "target", "counts", "nll", "flags", "ws"):
        assert finish(**{name: None}) == ERR_INVALID, name
    for name in ("B", "H", "W", "K"):
        assert finish(**{name: 0}) == ERR_INVALID, name
    assert finish(K=32768) == ERR_UNSUPPORTED
    assert lib.lseg_op_stats_finish_ws_bytes(0, 4, 4) == 0


# ---- the wrappers' argument checks: raised before the library is loaded or a kernel runs ---------------------------------------------------------
def test_wrappers_refuse_cpu_tensors_and_mismatched_shapes():
    from lseg_hip import metrics
    lab = torch.zeros((2, 4, 4), dtype=torch.int16)
    tgt = torch.zeros((2, 4, 4), dtype=torch.int64)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        metrics.label_stats(lab, tgt, 3)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        metrics.seg_stats_labels(lab, tgt, 3)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        metrics.SegmentationMetric(3).update_labels(tgt, lab)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        metrics.PanelStats(tgt, 3)
    with pytest.raises(TypeError):
        metrics.label_stats(lab.numpy(), tgt, 3)
    with pytest.raises(ValueError, match="masks for"):
        metrics.SegmentationMetric(3).update_labels([tgt], [lab, lab])


def test_wrapper_argument_checks_come_before_the_device_check_and_load_nothing(monkeypatch):
    """shape, dtype, list and map checks on plain host tensors: each raises its own error, none reaches the device check or loads the
    library; the same arguments made valid then stop at the device check"""
    from lseg_hip import metrics
    monkeypatch.setattr(_lib, "load", lambda: (_ for _ in ()).throw(AssertionError("the library was loaded")))
    lab, tgt = torch.zeros((2, 4, 4), dtype=torch.int16), torch.zeros((2, 4, 4), dtype=torch.int64)
    with pytest.raises(ValueError, match=r"must both be \[B,H,W\]"):
        metrics.label_stats(lab, torch.zeros((2, 4, 5), dtype=torch.int64), 3)
    with pytest.raises(ValueError, match="integer"):
        metrics.label_stats(lab, torch.zeros((2, 4, 4)), 3)
    with pytest.raises(ValueError, match="K "):
        metrics.label_stats(lab, tgt)
    with pytest.raises(ValueError, match="label lists"):
        metrics.label_stats(lab, tgt, group_sizes=[3, 5, 1])                    # three lists, two images
    with pytest.raises(ValueError, match="label lists"):
        metrics.label_stats(lab, tgt, group_sizes=[3, 0])
    with pytest.raises(ValueError, match="belongs to per-image"):
        metrics.label_stats(lab, tgt, 3, class_map=[0, 1, 2], nclass=3)
    with pytest.raises(ValueError, match="nclass"):
        metrics.label_stats(lab, tgt, group_sizes=[1, 2], class_map=[0, 1, 2])
    with pytest.raises(ValueError, match="out of range"):
        metrics.label_stats(lab, tgt, group_sizes=[1, 2], class_map=[0, 1, 5], nclass=3)
    with pytest.raises(ValueError, match="ids in"):
        metrics.label_stats(lab, tgt, group_sizes=[1, 2], class_map=[0, 1], nclass=3)
    with pytest.raises(ValueError, match="out must be"):
        metrics.label_stats(lab, tgt, 3, out=(torch.zeros(5, dtype=torch.int64), torch.zeros(2, dtype=torch.int64)))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        metrics.label_stats(lab, tgt, group_sizes=[1, 2], class_map=[0, 1, 2], nclass=3)
    with pytest.raises(ValueError, match="even H, W"):
        metrics.PanelStats(torch.zeros((2, 5, 4), dtype=torch.int64), 3)
    with pytest.raises(ValueError, match="K="):
        metrics.PanelStats(tgt, 0)


def test_engine_label_stats_argument_checks(monkeypatch):
    """HipEngine.label_stats' own checks need no engine: the method is called on a stand-in that has the attributes it reads"""
    import types
    from lseg_hip.engine import HipEngine
    monkeypatch.setattr(_lib, "load", lambda: (_ for _ in ()).throw(AssertionError("the library was loaded")))
    lab, tgt = torch.zeros((2, 4, 4), dtype=torch.int16), torch.zeros((2, 4, 4), dtype=torch.int64)
    eng = types.SimpleNamespace(device=torch.device("cuda", 0), _groups=None, _group=0, _K=3)
    with pytest.raises(TypeError):
        HipEngine.label_stats(eng, lab.numpy(), tgt)
    with pytest.raises(ValueError, match="must live on"):
        HipEngine.label_stats(eng, lab, tgt)                                    # host tensors for a device engine
    host = types.SimpleNamespace(device=torch.device("cpu"), _groups=[1, 2, 3], _group=0, _K=6)
    with pytest.raises(ValueError, match="label lists"):
        HipEngine.label_stats(host, lab, tgt)                                   # the engine's three ragged lists, two images
    host._groups = [1, 2]
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        HipEngine.label_stats(host, lab, tgt)                                   # everything valid but the device


# ---- declared, bound, exported -------------------------------------------------------------------------------------------------------------------
def _header_arity(name):
    src = open(os.path.join(_ROOT, "include", "lseg_hip.h")).read()
    m = re.search(r"\b(?:int|size_t)\s+" + name + r"\s*\(([^)]*)\)\s*;", src)
    assert m, f"{name} is not declared in include/lseg_hip.h"
    return len([p for p in re.sub(r"/\*.*?\*/", "", m.group(1)).split(",") if p.strip()])


@pytest.mark.parametrize("name,arity", [("lseg_op_label_stats_plan", 2), ("lseg_op_label_stats", 14), ("lseg_op_stats_fold_lowres", 13),
                                        ("lseg_op_stats_finish_ws_bytes", 3), ("lseg_op_stats_finish", 16)])
def test_new_entries_are_declared_bound_and_exported_with_matching_arity(name, arity):
    assert name in _lib.SIGNATURES
    assert len(_lib.SIGNATURES[name][1]) == arity == _header_arity(name)
    assert hasattr(_lib.load(), name)
