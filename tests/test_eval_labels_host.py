"""Host-side checks of the label panels of the multi-scale evaluator (BatchedMultiEval.forward_labels): plan_panels covers a label set
without gaps or overlap; the recurrence lseg_op_eval_merge_labels implements, restated in numpy (tests/eval_labels_helpers.py), gives
entries 0 / 1 of the stable descending sort and the log-sum-exp for every panel partition, on planes with planted ties; and the new
entries are declared, bound and exported."""
import os
import re

import numpy as np
import pytest
import torch

from eval_labels_helpers import PARTITIONS, merge_partition, planted_planes, stable_sort_reference
from lseg_hip import _lib
from lseg_hip.evaluator import plan_panels

_ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("K,panel", [(1, 64), (5, 64), (64, 64), (129, 64), (160, 7), (37, 1)])
def test_plan_panels_covers_the_label_set_without_gaps_or_overlap(K, panel):
    panels = plan_panels(K, panel)
    assert all(isinstance(r0, int) and isinstance(n, int) for r0, n in panels)
    assert panels[0][0] == 0 and all(1 <= n <= panel for _, n in panels)
    for (a0, an), (b0, _) in zip(panels, panels[1:]):
        assert a0 + an == b0                                   # ascending, no gap, no overlap
    assert panels[-1][0] + panels[-1][1] == K
    assert len(panels) == -(-K // panel)
    assert all(n == panel for _, n in panels[:-1])             # only the last panel may be short


def test_plan_panels_refuses_empty_sets_and_panels():
    for K, panel in ((0, 64), (5, 0), (-1, 3)):
        with pytest.raises(ValueError):
            plan_panels(K, panel)


def _partitions():
    return [(K, part) for K, parts in PARTITIONS.items() for part in parts]


@pytest.mark.parametrize("K,partition", _partitions(), ids=lambda p: "-".join(map(str, p))[:24] if isinstance(p, list) else str(p))
def test_merge_recurrence_equals_the_stable_sort_for_every_partition(K, partition):
    for seed, (H, W) in enumerate(((5, 7), (3, 29))):
        planes = planted_planes(K, H, W, seed, partition)
        if K >= 2:                                             # the plants are there: equal maxima, and a last plane equal to the winner
            assert ((planes == planes.max(dim=0).values).sum(dim=0) >= 2).any()
            assert (planes[K - 1] == planes.max(dim=0).values).any()
        lab, score, lab2, score2, lse = merge_partition(planes.numpy(), partition)
        rl, rs, rl2, rs2, rlse = stable_sort_reference(planes)
        assert np.array_equal(lab, rl.numpy()) and np.array_equal(lab2, rl2.numpy())
        assert np.array_equal(score, rs.double().numpy()) and np.array_equal(score2, rs2.double().numpy())
        assert np.abs(lse - rlse.numpy()).max() <= 1e-12


def test_every_partition_gives_the_same_state():
    planes = planted_planes(37, 4, 9, 3, [16, 16, 5]).numpy()
    want = merge_partition(planes, [37])
    for part in ([1] * 37, [16, 16, 5], [36, 1], [1, 36], [7] * 5 + [2]):
        got = merge_partition(planes, part)
        for a, b in zip(got[:4], want[:4]):
            assert np.array_equal(a, b), part
        assert np.abs(got[4] - want[4]).max() <= 1e-12


def test_single_label_has_no_runner_up():
    lab, score, lab2, score2, lse = merge_partition(np.array([[0.25]]), [1])
    assert (lab[0], score[0], lab2[0], score2[0], lse[0]) == (0, 0.25, -1, -np.inf, 0.25)


def _header_arity(name):
    src = open(os.path.join(_ROOT, "include", "lseg_hip.h")).read()
    m = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)\s*;", src)
    assert m, f"{name} is not declared in include/lseg_hip.h"
    return len([p for p in m.group(1).split(",") if p.strip()])


@pytest.mark.parametrize("name,arity", [("lseg_features_bytes", 4), ("lseg_forward_features", 6), ("lseg_score_features", 8),
                                        ("lseg_op_eval_merge_labels", 13)])
def test_new_entries_are_declared_bound_and_exported_with_matching_arity(name, arity):
    assert name in _lib.SIGNATURES
    assert len(_lib.SIGNATURES[name][1]) == _header_arity(name) == arity
    assert hasattr(_lib.load(), name)
    assert _lib.load().lseg_abi_version() == 1                 # additive: the ABI version stays


def test_forward_labels_needs_the_two_module_methods():
    """a module without hold_features / score_held: AttributeError, no fallback (checked before the device is touched)"""
    from lseg_hip.evaluator import BatchedMultiEval

    class Plain(torch.nn.Module):
        crop_size, base_size, mean, std = 64, 72, [0.5] * 3, [0.5] * 3
        _up_kwargs = {"mode": "bilinear", "align_corners": True}

        def evaluate(self, x, target=None):
            raise AssertionError("forward_labels must not fall back to the logits")

    ev = BatchedMultiEval(Plain(), 5)
    with pytest.raises(AttributeError, match="hold_features"):
        ev.forward_labels(torch.zeros(1, 3, 80, 104))
