"""Ragged training step, the parts that need no GPU: the launch plan of csrc/ragged_train.hip (lseg_op_ragged_ce_plan), the Python
argument checks, and the float64 restatement of the ragged loss (tests/ragged_train_helpers.py) pinned against a per-image
F.interpolate + F.cross_entropy loop -- the GPU tests take that restatement as their reference."""
import ctypes as C

import pytest
import torch
import torch.nn.functional as F

from lseg_hip import _lib
from lseg_hip.engine import check_group_sizes, check_ragged_target
from ragged_train_helpers import make_planes, make_targets, prefix_of, ragged_loss_f64, ragged_rows_reference, upsample2x_f64


def _plan(counts, h=24, w=20):
    lib = _lib.load()
    out = (C.c_int * 8)()
    r = lib.lseg_op_ragged_ce_plan((C.c_int32 * len(counts))(*counts), len(counts), h, w, out)
    return r, list(out)


@pytest.mark.parametrize("counts", [[1], [8, 9], [1, 9, 70]])
def test_plan_geometry(counts):
    r, p = _plan(counts)
    assert r == 0
    B, h, w = len(counts), 24, 20
    up64 = lambda v: (v + 63) // 64 * 64
    assert p[0] == sum(counts) and p[1] == max(counts)
    assert p[2] == up64(max(counts))                                   # one row pitch for the batch
    assert p[3] == min((B * 4 * h * w + 255) // 256, 4096)             # forward: 256 full-resolution pixels per workgroup, grid-stride
    assert p[4] == (B * h * w + 255) // 256                            # backward: one lane per low-resolution pixel
    assert p[5] == 256
    assert p[6] == sum(up64(k) for k in counts)                        # per-image transposed text panels, padded to the GEMM's K-step
    assert p[7] == sum(counts) * h * w == prefix_of(counts)[-1] * h * w


def test_plan_refuses_bad_counts_without_a_device():
    assert _plan([3, 0])[0] == -1 and _plan([40000])[0] == -1 and _plan([])[0] == -1
    assert _plan([2, 2], h=1)[0] == -1
    lib = _lib.load()
    assert lib.lseg_op_ragged_ce_plan(None, 2, 24, 20, (C.c_int * 8)()) == -1
    assert lib.lseg_op_ragged_ce_plan((C.c_int32 * 1)(1), 1, 24, 20, None) == -1


def test_group_size_checks():
    assert check_group_sizes([1, 9, 70], 80) == [1, 9, 70]
    with pytest.raises(ValueError, match="empty"):
        check_group_sizes([], 80)
    with pytest.raises(ValueError, match=">= 1 label"):
        check_group_sizes([3, 0, 2], 80)
    with pytest.raises(ValueError, match="max_labels"):
        check_group_sizes([81], 80)
    with pytest.raises(ValueError, match="in all"):
        check_group_sizes([50, 50], 80)


def test_target_checks():
    check_ragged_target(torch.zeros(3, 8, 6, dtype=torch.int64), 3, 8, 6)
    with pytest.raises(ValueError, match="int64"):
        check_ragged_target(torch.zeros(3, 8, 6, dtype=torch.int32), 3, 8, 6)
    with pytest.raises(ValueError, match=r"\[B,H,W\]"):
        check_ragged_target(torch.zeros(2, 8, 6, dtype=torch.int64), 3, 8, 6)
    with pytest.raises(ValueError, match="int64"):
        check_ragged_target([[0]], 1, 1, 1)


def test_network_argument_checks():
    """LSegNet: the list-of-lists form is recognised, forward refuses it naming forward_loss, forward_loss checks the list count."""
    from modules.models.lseg_net import LSegNet
    assert LSegNet._is_label_lists([["a"], ["b", "c"]]) and not LSegNet._is_label_lists(["a", "b"]) and not LSegNet._is_label_lists("")
    net = LSegNet.__new__(LSegNet)
    torch.nn.Module.__init__(net)
    net.train()
    x = torch.zeros(2, 3, 8, 8)
    with pytest.raises(ValueError, match="forward_loss"):
        net.forward(x, [["a"], ["b", "c"]])
    with pytest.raises(ValueError, match="3 lists"):
        net.forward_loss(x, torch.zeros(2, 8, 8, dtype=torch.int64), [["a"], ["b"], ["c"]])
    with pytest.raises(ValueError, match=">= 1 label"):
        net.forward_loss(x, torch.zeros(2, 8, 8, dtype=torch.int64), [["a"], []])
    with pytest.raises(ValueError, match="int64"):
        net.forward_loss(x, torch.zeros(2, 8, 8), [["a"], ["b", "c"]])


def test_upsample_restatement_is_interpolate():
    p = torch.randn(5, 7, 6, dtype=torch.float64, generator=torch.Generator().manual_seed(1))
    ref = F.interpolate(p[None], scale_factor=2, mode="bilinear", align_corners=True)[0]
    assert (upsample2x_f64(p) - ref).abs().max().item() <= 1e-13


@pytest.mark.parametrize("ignored_image", [None, 0])
def test_ragged_loss_restatement_against_per_image_cross_entropy(ignored_image):
    counts, h, w = [1, 9, 70], 12, 10
    planes = [p.double() for p in make_planes(counts, h, w, seed=3)]
    target = make_targets(counts, 2 * h, 2 * w, seed=4, ignored_image=ignored_image)
    leaves = [p.clone().requires_grad_(True) for p in planes]
    nll, valid = 0.0, 0
    for b, p in enumerate(leaves):
        out = F.interpolate(p[None], scale_factor=2, mode="bilinear", align_corners=True)
        nll = nll + F.cross_entropy(out, target[b:b + 1], ignore_index=-100, reduction="sum")
        valid += int((target[b] != -100).sum())
    (nll / valid).backward()
    got_nll, got_valid, lses = ragged_loss_f64(planes, target)
    assert got_valid == valid and abs(float(got_nll) - float(nll.detach())) <= 1e-10 * abs(float(nll.detach()))
    loss, _, _, _, rows = ragged_rows_reference(planes, target, ldk=128)
    assert abs(loss - float(nll) / valid) <= 1e-12
    for b, p in enumerate(leaves):
        ref = p.grad.reshape(counts[b], h * w).t()
        blk = rows[b * h * w:(b + 1) * h * w]
        assert (blk[:, :counts[b]] - ref).abs().max().item() <= 1e-15
        assert (blk[:, counts[b]:] == 0).all()
    if ignored_image is not None:
        assert (rows[:h * w] == 0).all()                           # an entirely ignored image gets no gradient
    # a target outside [0, k_b) that is not ignore_index contributes nothing (the kernels' rule for a target >= K)
    t2 = target.clone()
    t2[1][t2[1] == 3] = 9
    n2, v2, _ = ragged_loss_f64(planes, t2)
    assert v2 == valid - int((target[1] == 3).sum()) and float(n2) < float(got_nll)


def test_correlation_plan_geometry():
    lib = _lib.load()
    out = (C.c_int * 8)()
    up64 = lambda v: (v + 63) // 64 * 64
    for counts in ([1], [8, 9], [1, 9, 70]):
        B = len(counts)
        assert lib.lseg_op_corr_ragged_plan((C.c_int32 * B)(*counts), B, 480, 768, out) == 0
        # stage one: B GEMMs forward, B GEMMs + one L2-norm backward; stage two: one launch each, 64 / 16 pixel rows per workgroup
        assert list(out) == [B, B + 1, sum(up64(k) for k in counts), up64(max(counts)), sum(counts), B * 480 * 768, B * 8, B * 30]
    assert lib.lseg_op_corr_ragged_plan((C.c_int32 * 1)(3), 1, 480, 96, out) == -5        # C % 64
    assert lib.lseg_op_corr_ragged_plan((C.c_int32 * 1)(3), 1, 480, 1088, out) == -5      # C > 1024
    assert lib.lseg_op_corr_ragged_plan((C.c_int32 * 2)(3, 0), 2, 480, 128, out) == -1
