"""Segmentation statistics without the score planes (csrc/label_stats.hip): lseg_op_label_stats against the numpy reference and against
lseg_op_seg_stats of scores with the same arg-max; lseg_op_stats_fold_lowres / lseg_op_stats_finish against the CPU arg-max / gather of
the upsampled planes, lseg_op_seg_stats_lowres' counts and the float64 NLL within the counted bound; and the Python surface on top
(forward_metrics(panel=), label_metrics, SegmentationMetric.update_labels, BatchedMultiEval.parallel_forward_metrics)."""
import ctypes as C
import dataclasses
import functools
import os
import warnings

import numpy as np
import pytest
import torch

from label_stats_helpers import (emu_up2, fold_planes, fold_targets, nll_bound, partition_of, random_case, ref_label_stats, ref_nll)

pytestmark = [pytest.mark.gpu, pytest.mark.gpu_fast]

ERR_UNSUPPORTED = -5
LDS_BINS = 48 * 1024 // 12                                     # the largest bin count of the LDS route; LDS_BINS + 1 is the global route's smallest
GUARD = 0x7777
IGNORE = 255
_ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _P(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _lib():
    from lseg_hip import _lib
    return _lib, _lib.load()


def _offset_view(a, off):
    """a copy of `a` that starts `off` elements into its (256-byte aligned) allocation"""
    buf = torch.zeros(a.numel() + 16, dtype=a.dtype, device="cuda")
    buf[off:off + a.numel()] = a.reshape(-1)
    return buf[off:off + a.numel()].view(a.shape)


def _run_label_stats(lab, tgt, K, ignore_index, sizes=None, cmap=None, nclass=0, off=0, out=None):
    """the bare op on numpy inputs; counts / flags sit between guard words.  -> (counts, flags, guards intact, the two buffers)"""
    _l, lib = _lib()
    B, H, W = lab.shape
    n = nclass if cmap is not None else (sum(sizes) if sizes is not None else K)
    d_lab = _offset_view(torch.from_numpy(lab).cuda(), off)
    d_tgt = _offset_view(torch.from_numpy(tgt).cuda(), off)
    assert d_lab.data_ptr() % 8 == (2 * off) % 8 and d_tgt.data_ptr() % 16 == (8 * off) % 16
    if out is None:
        cbuf = torch.full((2 + 3 * n + 8,), GUARD, dtype=torch.int64, device="cuda")
        fbuf = torch.full((2 + 8,), GUARD, dtype=torch.int64, device="cuda")
    else:
        cbuf, fbuf = out
    d_off = torch.tensor([0] + list(np.cumsum(sizes)), dtype=torch.int32, device="cuda") if sizes is not None else None
    d_map = torch.tensor(cmap, dtype=torch.int32, device="cuda") if cmap is not None else None
    _l.check(lib.lseg_op_label_stats(_P(d_lab), _P(d_tgt), B, H, W, K if sizes is None else max(sizes), ignore_index, _P(d_off), _P(d_map), nclass,
                                     _P(cbuf[4:]), _P(fbuf[4:]), int(out is not None), _stream()))
    torch.cuda.synchronize()
    c, f = cbuf.cpu().numpy(), fbuf.cpu().numpy()
    clean = (c[:4] == GUARD).all() and (c[-4:] == GUARD).all() and (f[:4] == GUARD).all() and (f[-4:] == GUARD).all()
    return c[4:-4], f[4:-4], bool(clean), (cbuf, fbuf)


def _seg_stats_counts(lab, tgt, K):
    """lseg_op_seg_stats on random scores whose first-maximum arg-max is `lab` (the label's score raised above the others; a second,
    LATER entry equal to it where there is room: the first maximum still wins)"""
    _l, lib = _lib()
    B, H, W = lab.shape
    g = torch.Generator().manual_seed(K + H)
    scores = torch.rand((B, K, H, W), generator=g) * 2 - 1
    idx = torch.from_numpy(lab.astype(np.int64))[:, None]
    scores.scatter_(1, idx, 2.0)
    later = torch.clamp(idx + 1, max=K - 1)
    scores.scatter_(1, later, 2.0)                              # equal to the winner and behind it (or the winner itself at K - 1)
    assert torch.equal(scores.argmax(1), idx[:, 0])
    d_s, d_t = scores.cuda(), torch.from_numpy(tgt).cuda()
    counts = torch.empty(2 + 3 * K, dtype=torch.int64, device="cuda")
    nll = torch.empty(2, dtype=torch.float64, device="cuda")
    _l.check(lib.lseg_op_seg_stats(_P(d_s), _P(d_t), B, K, H, W, -1, _P(counts), _P(nll), _stream()))
    torch.cuda.synchronize()
    return counts.cpu().numpy()


def _route(bins):
    _l, lib = _lib()
    out = (C.c_int * 2)()
    assert lib.lseg_op_label_stats_plan(bins, out) == 0
    return out[0]


SHAPES = [(1, 1), (6, 10), (7, 13), (64, 64)]
KS = [1, 2, 7, 300, LDS_BINS, LDS_BINS + 1, 32767]


@pytest.mark.parametrize("K", KS)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("B", [1, 3])
def test_label_stats_shared_set(B, shape, K):
    """exact equality with the numpy reference at an unaligned view (one element in: the 8-byte label words and 16-byte target words
    start elsewhere, heads and tails run element by element) with accumulate = 0, then accumulate = 1 on an aligned copy doubles every
    word; and the kernel's output with ignore_index = -1, on the same targets with 255 turned into -1 (the one target value the two ops
    read differently), equals lseg_op_seg_stats of scores with that arg-max (its K <= 4096; score tensors up to 64 MB)"""
    H, W = shape
    assert _route(K) == (0 if K <= LDS_BINS else 1)
    lab, tgt = random_case(B, H, W, [K] * B, seed=K + 31 * H + B, ignore_index=IGNORE)
    ref_c, ref_f = ref_label_stats(lab, tgt, K, IGNORE)
    c, f, clean, bufs = _run_label_stats(lab, tgt, K, IGNORE, off=1)
    assert clean
    assert np.array_equal(c, ref_c), np.flatnonzero(c != ref_c)[:8]
    assert np.array_equal(f, ref_f), (f, ref_f)
    c2, f2, clean, _ = _run_label_stats(lab, tgt, K, IGNORE, off=0, out=bufs)
    assert clean and np.array_equal(c2, 2 * ref_c) and np.array_equal(f2, 2 * ref_f)
    if K <= 4096 and B * K * H * W <= 2 ** 24:                  # lseg_op_seg_stats' K; the score tensor up to 64 MB (K = 4096 at 64 x 64: B = 1)
        t_ss = np.where(tgt == IGNORE, -1, tgt)
        c_ss, f_ss, clean, _ = _run_label_stats(lab, t_ss, K, -1, off=1)       # the kernel itself, ignore_index = -1, on those targets
        assert clean and np.array_equal(c_ss, c) and np.array_equal(f_ss, f)
        assert np.array_equal(c_ss, _seg_stats_counts(lab, t_ss, K))


def test_label_stats_counts_labels_outside_their_range():
    lab, tgt = random_case(2, 7, 13, [7, 7], seed=2, ignore_index=IGNORE, bad_labels=True)
    ref_c, ref_f = ref_label_stats(lab, tgt, 7, IGNORE)
    assert ref_f[1] > 0
    c, f, clean, _ = _run_label_stats(lab, tgt, 7, IGNORE)
    assert clean and np.array_equal(c, ref_c) and np.array_equal(f, ref_f)


@pytest.mark.parametrize("shape", [(1, 1), (7, 13), (64, 64)], ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("sizes", [(3, 5), (1, 9, 2)], ids=lambda s: "_".join(map(str, s)))
def test_label_stats_ragged_and_mapped(sizes, shape):
    """ragged lists: areas indexed offsets[b] + l; then through a class map with duplicates (inside a list and across lists) and one id
    outside [0, nclass), which reaches no bin and writes nowhere; accumulate = 1 on top doubles every word"""
    H, W = shape
    sizes = list(sizes)
    B, n = len(sizes), sum(sizes)
    lab, tgt = random_case(B, H, W, sizes, seed=n + H, ignore_index=IGNORE)
    for off in (0, 1):
        ref_c, ref_f = ref_label_stats(lab, tgt, ignore_index=IGNORE, group_sizes=sizes)
        c, f, clean, bufs = _run_label_stats(lab, tgt, None, IGNORE, sizes=sizes, off=off)
        assert clean and np.array_equal(c, ref_c) and np.array_equal(f, ref_f), off
    c2, f2, clean, _ = _run_label_stats(lab, tgt, None, IGNORE, sizes=sizes, out=bufs)
    assert clean and np.array_equal(c2, 2 * ref_c) and np.array_equal(f2, 2 * ref_f)
    nclass = 4
    cmap = [(3 * i + 1) % nclass for i in range(n)]
    cmap[1] = cmap[0]                                           # a duplicate inside image 0's list (where it has two entries) / across lists
    cmap[n - 2] = nclass + 2                                    # outside [0, nclass)
    for nc, route in ((nclass, 0), (LDS_BINS + 1, 1)):          # the same ids in a vocabulary on either side of the LDS budget
        ref_c, ref_f = ref_label_stats(lab, tgt, ignore_index=IGNORE, group_sizes=sizes, class_map=cmap, nclass=nc)
        assert _route(nc) == route
        c, f, clean, _ = _run_label_stats(lab, tgt, None, IGNORE, sizes=sizes, cmap=cmap, nclass=nc, off=1)
        assert clean and np.array_equal(c, ref_c) and np.array_equal(f, ref_f), nc


# ---- fold / finish ----------------------------------------------------------------------------------------------------------------------------
def _up2_device(low):
    """lseg_op_upsample2x_planes of the planes (it takes W % 4 == 0), on the CPU afterwards"""
    _l, lib = _lib()
    B, K, h, w = low.shape
    d = torch.from_numpy(low).cuda()
    out = torch.empty((B, K, 2 * h, 2 * w), device="cuda")
    _l.check(lib.lseg_op_upsample2x_planes(_P(d), _P(out), B * K, h, w, _stream()))
    torch.cuda.synchronize()
    return out.cpu().numpy()


def _fold_finish(low, tgt, partition, ignore_index=-1):
    _l, lib = _lib()
    B, K, h, w = low.shape
    H, W = 2 * h, 2 * w
    d_t = torch.from_numpy(tgt).cuda()
    label = torch.full((B, H, W), 77, dtype=torch.int16, device="cuda")
    best, s, tl = (torch.full((B, H, W), 777.0, device="cuda") for _ in range(3))
    row0 = 0
    for rows in partition:
        panel = torch.from_numpy(np.ascontiguousarray(low[:, row0:row0 + rows])).cuda()
        _l.check(lib.lseg_op_stats_fold_lowres(_P(panel), B, rows, row0, h, w, _P(d_t), _P(label), _P(best), _P(s), _P(tl), int(row0 == 0), _stream()))
        row0 += rows
    nws = lib.lseg_op_stats_finish_ws_bytes(B, H, W)
    assert nws >= 16 * B
    ws = torch.empty(nws // 8, dtype=torch.float64, device="cuda")
    outs = []
    for _ in range(2):                                          # two runs: the same nll bits
        cbuf = torch.full((2 + 3 * K + 8,), GUARD, dtype=torch.int64, device="cuda")
        fbuf = torch.full((3 + 8,), GUARD, dtype=torch.int64, device="cuda")
        nll = torch.full((2,), 777.0, dtype=torch.float64, device="cuda")
        _l.check(lib.lseg_op_stats_finish(_P(label), _P(best), _P(s), _P(tl), _P(d_t), B, H, W, K, ignore_index, _P(cbuf[4:]), _P(nll), _P(fbuf[4:]),
                                          _P(ws), nws, _stream()))
        torch.cuda.synchronize()
        c, f = cbuf.cpu().numpy(), fbuf.cpu().numpy()
        assert (c[:4] == GUARD).all() and (c[-4:] == GUARD).all() and (f[:4] == GUARD).all() and (f[-4:] == GUARD).all()
        outs.append((c[4:-4], nll.cpu().numpy(), f[4:-4]))
    assert outs[0][1].tobytes() == outs[1][1].tobytes() and np.array_equal(outs[0][0], outs[1][0])
    state = tuple(x.cpu().numpy() for x in (label, best, s, tl))
    return state, outs[0]


FOLD_HW = [(2, 2), (3, 5), (4, 4), (16, 12)]
FOLD_K = [1, 7, 37]
FOLD_KINDS = ["rand", "ramp", "flat"]


@functools.lru_cache(maxsize=None)
def _fold_case(h, w, K, kind):
    """one case of test_fold_and_finish, every assertion included; -> {panel size: NLL error / counted bound}.  Cached, so that the
    ratio report reads the cases that ran and runs the ones that were deselected."""
    _l, lib = _lib()
    B, H, W = 2, 2 * h, 2 * w
    panels = sorted({1, 5, 16, K} & set(range(1, K + 1)) | {K})
    low = fold_planes(B, K, h, w, kind, seed=K + h, partition=partition_of(K, 5))
    up = emu_up2(low)
    if w % 4 == 0:
        assert np.array_equal(_up2_device(low), up)
    tgt = fold_targets(B, K, H, W, partition_of(K, 5), seed=K + w)
    valid = tgt >= 0
    want_label = up.argmax(axis=1).astype(np.int16)             # numpy: the first maximum
    want_best = up.max(axis=1)
    want_tl = np.take_along_axis(up, np.clip(tgt, 0, K - 1)[:, None], axis=1)[:, 0]
    if kind == "rand" and K >= 2:
        assert ((up == want_best[:, None]).sum(axis=1) >= 2).any()
    nsum, ncount, m64, px64, v64 = ref_nll(up, tgt)
    bound = nll_bound(K, m64, px64, v64)
    # lseg_op_seg_stats_lowres' counts for the same planes and targets
    d_low, d_t = torch.from_numpy(low).cuda(), torch.from_numpy(tgt).cuda()
    ss_counts = torch.empty(2 + 3 * K, dtype=torch.int64, device="cuda")
    ss_nll = torch.empty(2, dtype=torch.float64, device="cuda")
    _l.check(lib.lseg_op_seg_stats_lowres(_P(d_low), _P(d_t), B, K, h, w, -1, _P(ss_counts), _P(ss_nll), None, _stream()))
    torch.cuda.synchronize()
    first, ratios = None, {}
    for p in panels:
        (label, best, s, tl), (counts, nll, flags) = _fold_finish(low, tgt, partition_of(K, p))
        assert np.array_equal(label, want_label), p
        assert best.tobytes() == want_best.tobytes(), p
        assert tl[valid].tobytes() == want_tl[valid].tobytes() and np.isnan(tl[~valid]).all(), p
        if first is None:
            first = (label, best, s, tl, counts, nll)
        else:                                                   # the state is identical for every panel size
            assert s.tobytes() == first[2].tobytes() and np.array_equal(counts, first[4]) and nll.tobytes() == first[5].tobytes(), p
        assert np.array_equal(counts, ss_counts.cpu().numpy()), p
        assert np.array_equal(counts, ref_label_stats(want_label, tgt, K, -1)[0])
        assert flags.tolist() == [0, 0, 0] and nll[1] == ncount == int(valid.sum())
        err = abs(nll[0] - nsum)
        ratio = err / bound
        ratios[p] = ratio
        print(f"{h}x{w} K={K} {kind} panel={p}: |nll - fp64| = {err:.3e}, bound {bound:.3e}, ratio {ratio:.3f}")
        assert err <= bound, (err, bound)
    return ratios


@pytest.mark.parametrize("kind", FOLD_KINDS)
@pytest.mark.parametrize("K", FOLD_K)
@pytest.mark.parametrize("hw", FOLD_HW, ids=lambda s: f"{s[0]}x{s[1]}")
def test_fold_and_finish(hw, K, kind):
    """panels of 1 / 5 / 16 / K over planes with exact ties across the first panel boundary, an ascending ramp of +-80 (every label a new
    best: every step rescales the sum) and a flat set; targets on the panel edges.  The upsampled values are lseg_op_upsample2x_planes'
    where it runs (w % 4 == 0) -- and the CPU restatement of its arithmetic must equal them there bit for bit; at the other widths the
    restatement alone."""
    ratios = _fold_case(hw[0], hw[1], K, kind)
    assert ratios and max(ratios.values()) <= 1.0


def test_finish_counts_targets_no_panel_covered():
    """only labels 0 .. 4 of 7 are folded, then finish is told K = 7: valid pixels whose target is 5 or 6 have no logit -- counted in the
    third flag word and left out of the sum and the count"""
    _l, lib = _lib()
    low = fold_planes(1, 7, 4, 4, "rand", 3, [5, 2])
    tgt = fold_targets(1, 7, 8, 8, [5, 2], 3)
    d_t = torch.from_numpy(tgt).cuda()
    label = torch.empty((1, 8, 8), dtype=torch.int16, device="cuda")
    best, s, tl = (torch.empty((1, 8, 8), device="cuda") for _ in range(3))
    panel = torch.from_numpy(np.ascontiguousarray(low[:, :5])).cuda()
    _l.check(lib.lseg_op_stats_fold_lowres(_P(panel), 1, 5, 0, 4, 4, _P(d_t), _P(label), _P(best), _P(s), _P(tl), 1, _stream()))
    nws = lib.lseg_op_stats_finish_ws_bytes(1, 8, 8)
    ws = torch.empty(nws // 8, dtype=torch.float64, device="cuda")
    counts = torch.empty(2 + 21, dtype=torch.int64, device="cuda")
    flags = torch.empty(3, dtype=torch.int64, device="cuda")
    nll = torch.empty(2, dtype=torch.float64, device="cuda")
    _l.check(lib.lseg_op_stats_finish(_P(label), _P(best), _P(s), _P(tl), _P(d_t), 1, 8, 8, 7, -1, _P(counts), _P(nll), _P(flags), _P(ws), nws, _stream()))
    torch.cuda.synchronize()
    missing = int((tgt >= 5).sum())
    assert missing > 0 and flags.tolist() == [0, 0, missing]
    assert nll[1].item() == int(((tgt >= 0) & (tgt < 5)).sum())


def test_nll_ratios_are_written(repo_root):
    """the measured worst ratio of the NLL error to its counted bound, per shape, into profiles/label_stats.txt (the section between the
    markers is replaced; the rest of the file, the benchmark tool's, stays).  Independent of which other tests ran: the cases come from
    _fold_case's cache or are run here."""
    _RATIOS = {(h, w, K, kind, p): r for (h, w) in FOLD_HW for K in FOLD_K for kind in FOLD_KINDS for p, r in _fold_case(h, w, K, kind).items()}
    worst = max(_RATIOS.values())
    lines = ["## NLL error / counted bound (tests/test_gpu_label_stats.py::test_fold_and_finish)",
             f"worst ratio over {len(_RATIOS)} runs: {worst:.4f}"]
    for key in sorted({k[:2] for k in _RATIOS}):
        sub = {k: v for k, v in _RATIOS.items() if k[:2] == key}
        kmax = max(sub, key=sub.get)
        lines.append(f"  {key[0]}x{key[1]}: worst {sub[kmax]:.4f} at K={kmax[2]} {kmax[3]} panel={kmax[4]}")
    path = os.path.join(repo_root, "profiles", "label_stats.txt")
    begin, end = "<!-- nll-ratios:begin -->", "<!-- nll-ratios:end -->"
    old = open(path).read() if os.path.exists(path) else ""
    block = begin + "\n" + "\n".join(lines) + "\n" + end
    if begin in old and end in old:
        new = old[:old.index(begin)] + block + old[old.index(end) + len(end):]
    else:
        new = old + ("\n" if old and not old.endswith("\n") else "") + block + "\n"
    try:
        if new != old:                                          # the same figures: the file is left alone
            with open(path, "w") as fh:
                fh.write(new)
    except OSError as e:                                        # a read-only checkout: the figures are in the test's output
        print(f"could not write {path}: {e}")
    print("\n".join(lines))
    assert worst <= 1.0


# ---- the engine and the Python surface ----------------------------------------------------------------------------------------------------------
LABELS11 = [f"thing number {i}" for i in range(11)]


def _net(labels=LABELS11, image_dtype="fp16", cfg=None):
    from lseg_hip.config import get_config
    from lseg_hip.synth import synthetic_state_dict
    from modules.models.lseg_net import LSegNet
    cfg = cfg or get_config("tiny16")
    net = LSegNet(labels=labels, backbone="tiny16", features=cfg.features, arch_option=0, block_depth=0, activation="lrelu",
                  batch_invariant=True, image_dtype=image_dtype)
    net.load_state_dict(synthetic_state_dict(net.cfg, seed=2))
    return net.eval().cuda()


def _targets(B, H, W, K, seed):
    g = torch.Generator().manual_seed(seed)
    t = torch.randint(0, K, (B, H, W), generator=g)
    t[:, ::5, ::3] = -1
    t[:, 1, :] = K - 1
    return t.cuda()


def _same_counts(a, b):
    return (a["correct"] == b["correct"] and a["labeled"] == b["labeled"]
            and all(torch.equal(a[k].cpu(), b[k].cpu()) for k in ("area_inter", "area_pred", "area_lab", "area_union")))


@pytest.fixture(scope="module")
def tiny_run():
    """tiny16, 64 x 64, B = 2, K = 11, fp16 operands: forward_metrics on today's route, its low-resolution logits and the float64 NLL"""
    warnings.simplefilter("ignore")
    from lseg_hip.synth import synthetic_images
    net = _net()
    x = synthetic_images(2, 64, 64, seed=7).cuda()
    target = _targets(2, 64, 64, 11, 1)
    want = net.forward_metrics(x, target)
    with torch.no_grad():
        low = net.forward_lowres(x).cpu().numpy()
    up = emu_up2(low)
    nsum, ncount, m64, px64, v64 = ref_nll(up, target.cpu().numpy())
    return net, x, target, want, (nsum, ncount, nll_bound(11, m64, px64, v64))


@pytest.mark.parametrize("panel", [4, 11, 64])
def test_forward_metrics_panels_equal_forward_metrics(tiny_run, panel):
    net, x, target, want, (nsum, ncount, bound) = tiny_run
    got = net.forward_metrics(x, target, panel=panel)
    assert set(got) == set(want)
    assert _same_counts(got, want)
    assert got["nll_count"] == want["nll_count"] == ncount
    err = abs(got["nll_sum"] - nsum)
    print(f"panel={panel}: |nll - fp64| = {err:.3e} (bound {bound:.3e}); forward_metrics' own: {abs(want['nll_sum'] - nsum):.3e}")
    assert err <= bound


def test_forward_metrics_panel_sizes_the_engine_by_the_panel(tiny_run):
    """a network that has run nothing else: after forward_metrics(panel=4) over K = 11 labels its engine holds label planes for 4 labels
    (the engine's planes are max_batch x max_labels x H/2 x W/2), and the result is the one of the network whose engine holds all 11"""
    _, x, target, want, _ = tiny_run
    fresh = _net()
    got = fresh.forward_metrics(x, target, panel=4)
    assert len(fresh._engines) == 1 and fresh._last_engine.max_labels == 4
    assert _same_counts(got, want) and got["nll_count"] == want["nll_count"]
    got = fresh.forward_metrics(x, target, labelset=LABELS11, panel=5)          # a label list: tokenised once, sliced per panel
    assert fresh._last_engine.max_labels == 5 and _same_counts(got, want)


def test_label_metrics_shared_list_and_update_labels(tiny_run):
    from lseg_hip.metrics import SegmentationMetric
    from lseg_hip.synth import synthetic_images
    net, x, target, want, _ = tiny_run
    got = net.label_metrics(x, target)
    assert "nll_sum" not in got and got["flags"] == [0, 0]
    assert _same_counts(got, want)
    # SegmentationMetric.update_labels over two batches == update on the logits
    x2 = synthetic_images(2, 64, 64, seed=8).cuda()
    t2 = _targets(2, 64, 64, 11, 2)
    a, b = SegmentationMetric(11), SegmentationMetric(11)
    with torch.no_grad():
        for xi, ti in ((x, target), (x2, t2)):
            a.update(ti, net(xi))
            b.update_labels(ti, net.predict_labels(xi))
    assert a.total_correct == b.total_correct and a.total_label == b.total_label
    assert torch.equal(a.total_inter, b.total_inter) and torch.equal(a.total_union, b.total_union)
    assert a.get() == b.get()


def test_forward_metrics_panel_refusals(tiny_run):
    from lseg_hip import _lib
    net, x, target, _, _ = tiny_run
    with pytest.raises(_lib.LSegError) as e:
        net.forward_metrics(x, target, labelset=[["a", "b"], ["c"]], panel=4)
    assert e.value.code == ERR_UNSUPPORTED
    net.train()
    try:
        with pytest.raises(_lib.LSegError) as e:
            net.forward_metrics(x, target, panel=4)
        assert e.value.code == ERR_UNSUPPORTED
    finally:
        net.eval()


def test_label_metrics_per_image_lists(monkeypatch):
    """the synthetic small network widened to out_c = 512 (the streamed route), per-image lists of 2 / 5 / 9 labels: the ragged counts
    are the label_stats of one shared-set run per list, laid side by side; with class ids they add up per class"""
    warnings.simplefilter("ignore")
    from lseg_hip import config as lseg_config
    from lseg_hip.config import get_config
    from lseg_hip.metrics import seg_stats_labels
    from lseg_hip.synth import synthetic_images
    base = get_config("tiny16")
    cfg = dataclasses.replace(base, out_c=512, text=dataclasses.replace(base.text, embed_dim=512))
    monkeypatch.setitem(lseg_config._CONFIGS, "tiny16", cfg)
    net = _net(labels=["a", "b"], cfg=cfg)
    assert net.cfg.out_c == 512
    lists = [["cat", "grass"], ["road", "car", "sky", "tree", "wall"], [f"item {i}" for i in range(9)]]
    sizes = [len(ls) for ls in lists]
    n = sum(sizes)
    x = synthetic_images(3, 64, 64, seed=5).cuda()
    g = torch.Generator().manual_seed(4)
    target = torch.stack([torch.randint(-1, k, (64, 64), generator=g) for k in sizes]).cuda()
    got = net.label_metrics(x, target, lists)
    assert got["area_pred"].numel() == n and got["flags"] == [0, 0]
    correct = labeled = 0
    off = 0
    for b, ls in enumerate(lists):
        lab = net.predict_labels(x, ls)                         # the same batch against list b, shared
        r = seg_stats_labels(lab[b:b + 1], target[b:b + 1], len(ls))
        correct += r["correct"]
        labeled += r["labeled"]
        for k in ("area_inter", "area_pred", "area_lab"):
            assert torch.equal(got[k][off:off + len(ls)], r[k]), (b, k)
        off += len(ls)
    assert (got["correct"], got["labeled"]) == (correct, labeled)
    ids = [[0, 1], [2, 3, 4, 1, 0], [5, 5, 0, 1, 2, 3, 4, 5, 5]]
    mapped = net.label_metrics(x, target, lists, class_ids=ids, nclass=6)
    flat = [c for cs in ids for c in cs]
    for k in ("area_pred", "area_lab"):
        want = torch.zeros(6, dtype=torch.int64).index_add_(0, torch.tensor(flat), got[k])
        assert torch.equal(mapped[k], want), k
    assert mapped["labeled"] == labeled and mapped["correct"] >= correct


class _Mod(torch.nn.Module):
    def __init__(self, net, crop, base):
        super().__init__()
        self.net, self.crop_size, self.base_size = net, crop, base
        self.mean, self.std = [0.5, 0.5, 0.5], [0.5, 0.5, 0.5]
        self._up_kwargs = {"mode": "bilinear", "align_corners": True}

    def hold_features(self, x):
        return self.net.hold_features(x)

    def score_held(self, held, row0, rows, labelset=""):
        return self.net.score_held(held, row0, rows, labelset)


def test_parallel_forward_metrics_is_update_labels_of_forward_labels(tiny_run):
    from lseg_hip.evaluator import BatchedMultiEval
    from lseg_hip.metrics import SegmentationMetric
    from lseg_hip.synth import synthetic_images
    net = tiny_run[0]
    ev = BatchedMultiEval(_Mod(net, 64, 72), 11, flip=True, scales=(0.75, 1.0, 1.5), max_batch=8)
    img = torch.nn.functional.interpolate(synthetic_images(1, 64, 64, seed=9), (40, 56), mode="bilinear", align_corners=True)[0].cuda()
    tgt = _targets(1, 40, 56, 11, 5)[0]
    (r,) = ev.parallel_forward_metrics([img], [tgt], panel=4)
    label, _ = ev.forward_labels(img.unsqueeze(0), panel=64)
    m = SegmentationMetric(11)
    m.update_labels(tgt, label)
    assert (r["correct"], r["labeled"]) == (m.total_correct, m.total_label) and r["labeled"] > 0
    assert torch.equal(r["area_inter"], m.total_inter) and torch.equal(r["area_union"], m.total_union)
