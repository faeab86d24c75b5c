"""Device-side segmentation metrics and cross-entropy value (include/lseg_hip.h: lseg_op_seg_stats).

Replaces the host/numpy step the reference runs on the full [B,K,H,W] logits after every forward:
`batch_pix_accuracy`, `batch_intersection_union` ([3P] encoding/utils/metrics.py, called at
modules/lsegmentation_module.py:49-50,59-60) and the forward value of `SegmentationLosses` =
`nn.CrossEntropyLoss(ignore_index)` ([3P] encoding/nn/loss.py, called at :72).  One pass over the scores on the GPU;
no CPU fallback (CPU tensors raise).
"""
import ctypes as C

import torch

from . import _lib


def seg_stats(scores: torch.Tensor, target: torch.Tensor, ignore_index: int = -1) -> dict:
    """scores fp32 [B,K,H,W] (CUDA), target int64 [B,H,W] (-1 = unlabeled).  Returns python/CPU values:
    correct, labeled (ints), area_inter/area_pred/area_lab/area_union (int64 [K]), nll_sum, nll_count."""
    if not scores.is_cuda:
        raise RuntimeError("lseg_hip.metrics.seg_stats runs on the GPU (no CPU fallback): pass CUDA tensors")
    lib = _lib.load()
    B, K, H, W = scores.shape
    s = scores.detach().float().contiguous()
    t = target.detach().to(scores.device, torch.int64).contiguous()
    if tuple(t.shape) != (B, H, W):
        raise ValueError(f"target shape {tuple(t.shape)} != {(B, H, W)}")
    counts = torch.empty(2 + 3 * K, dtype=torch.int64, device=scores.device)
    nll = torch.empty(2, dtype=torch.float64, device=scores.device)
    st = torch.cuda.current_stream(scores.device).cuda_stream
    _lib.check(lib.lseg_op_seg_stats(C.c_void_p(s.data_ptr()), C.c_void_p(t.data_ptr()), B, K, H, W, int(ignore_index),
                                     C.c_void_p(counts.data_ptr()), C.c_void_p(nll.data_ptr()), C.c_void_p(st)))
    c = counts.cpu()
    n = nll.cpu()
    inter, pred, lab = c[2:2 + K], c[2 + K:2 + 2 * K], c[2 + 2 * K:2 + 3 * K]
    return {"correct": int(c[0]), "labeled": int(c[1]), "area_inter": inter, "area_pred": pred, "area_lab": lab,
            "area_union": pred + lab - inter, "nll_sum": float(n[0]), "nll_count": int(n[1])}


def _counts_dict(c: torch.Tensor, n: int) -> dict:
    inter, pred, lab = c[2:2 + n], c[2 + n:2 + 2 * n], c[2 + 2 * n:2 + 3 * n]
    return {"correct": int(c[0]), "labeled": int(c[1]), "area_inter": inter, "area_pred": pred, "area_lab": lab,
            "area_union": pred + lab - inter}


def label_stats(labels: torch.Tensor, target: torch.Tensor, K: int = None, ignore_index: int = -1, group_sizes=None, class_map=None,
                nclass: int = None, out=None):
    """The counters of a label map (lseg_op_label_stats), on the device and without a host synchronisation: (counts int64 [2 + 3n],
    flags int64 [2]) with n = K (one label set shared by the batch), sum(group_sizes) (ragged per-image lists: labels and targets index
    each image's own list, areas indexed offsets[b] + l) or nclass (ragged lists mapped into one vocabulary by class_map, one class id per
    list entry: per-image lists drawn from one vocabulary add up to per-class IoU).
    labels [B,H,W] int16 (or any integer dtype holding labels <= 32767), target [B,H,W] integer, both CUDA.  class_map is validated
    HERE, on the host (the caller picked the lists: it has the ids there); the kernel skips an id outside [0, nclass).
    out = (counts, flags) of an earlier call: this batch is ADDED to them (a meter that lives on the device)."""
    if not torch.is_tensor(labels) or not torch.is_tensor(target):
        raise TypeError("label_stats: labels and target must be tensors")
    if labels.dim() != 3 or tuple(target.shape) != tuple(labels.shape):
        raise ValueError(f"label_stats: labels {tuple(labels.shape)} and target {tuple(target.shape)} must both be [B,H,W]")
    if labels.dtype.is_floating_point or target.dtype.is_floating_point:
        raise ValueError("label_stats: labels and target must be integer tensors")
    B, H, W = labels.shape
    offsets = cmap = None
    if group_sizes is None:
        if class_map is not None:
            raise ValueError("label_stats: a class map belongs to per-image label lists (group_sizes)")
        if K is None or int(K) < 1:
            raise ValueError("label_stats: K (the size of the shared label set) is required")
        K = n = int(K)
    else:
        sizes = [int(g) for g in group_sizes]
        if len(sizes) != B or min(sizes) < 1:
            raise ValueError(f"label_stats: {len(sizes)} label lists (sizes {sizes}) for a batch of {B}; every image needs >= 1 label")
        K, n = max(sizes), sum(sizes)
        offs = [0]
        for g in sizes:
            offs.append(offs[-1] + g)
        if class_map is not None:
            ids = [int(c) for c in (class_map.tolist() if torch.is_tensor(class_map) else class_map)]
            if nclass is None or int(nclass) < 1:
                raise ValueError("label_stats: a class map needs nclass >= 1")
            bad = [c for c in ids if not 0 <= c < int(nclass)]
            if len(ids) != n or bad:
                raise ValueError(f"label_stats: class_map needs {n} ids in [0, nclass={nclass}); got {len(ids)} ids, out of range: {bad[:8]}")
            n = int(nclass)
            cmap = ids
        offsets = offs
    if out is not None:
        counts, flags = out
        if (counts.dtype != torch.int64 or flags.dtype != torch.int64 or counts.numel() != 2 + 3 * n or flags.numel() != 2
                or counts.device != labels.device or flags.device != labels.device or not counts.is_contiguous() or not flags.is_contiguous()):
            raise ValueError(f"label_stats: out must be (int64 [{2 + 3 * n}], int64 [2]) on {labels.device}")
    if not labels.is_cuda or not target.is_cuda:
        raise RuntimeError("lseg_hip.metrics.label_stats runs on the GPU (no CPU fallback): pass CUDA tensors")
    lib = _lib.load()
    lab = labels.detach().to(torch.int16).contiguous()
    if offsets is not None:
        offsets = torch.tensor(offsets, dtype=torch.int32).to(labels.device, non_blocking=True)
    if cmap is not None:
        cmap = torch.tensor(cmap, dtype=torch.int32).to(labels.device, non_blocking=True)
    t = target.detach().to(torch.int64).contiguous()
    if out is None:
        counts = torch.empty(2 + 3 * n, dtype=torch.int64, device=labels.device)
        flags = torch.empty(2, dtype=torch.int64, device=labels.device)
    P = lambda x: C.c_void_p(x.data_ptr()) if x is not None else None          # noqa: E731
    st = torch.cuda.current_stream(labels.device).cuda_stream
    _lib.check(lib.lseg_op_label_stats(P(lab), P(t), B, H, W, K, int(ignore_index), P(offsets), P(cmap), int(nclass) if cmap is not None else 0,
                                       P(counts), P(flags), int(out is not None), C.c_void_p(st)))
    return counts, flags


def seg_stats_labels(labels: torch.Tensor, target: torch.Tensor, K: int = None, ignore_index: int = -1, group_sizes=None, class_map=None,
                     nclass: int = None) -> dict:
    """seg_stats for a label map instead of the scores (label_stats above): the dict seg_stats returns without the nll_* keys -- a label map
    holds no loss -- plus "flags" (the two words of lseg_op_label_stats, python ints)."""
    counts, flags = label_stats(labels, target, K, ignore_index, group_sizes, class_map, nclass)
    c = counts.cpu()
    r = _counts_dict(c, (c.numel() - 2) // 3)
    r["flags"] = [int(f) for f in flags.cpu()]
    return r


class PanelStats:
    """seg_stats of low-resolution logits that arrive in label PANELS (lseg_op_stats_fold_lowres / lseg_op_stats_finish): the state is four
    [B,H,W] planes (14 bytes per pixel) whatever K is.  `fold(low, row0)` takes fp32 [B,rows,H/2,W/2] for labels row0 .. row0+rows-1 in
    ascending order; `finish()` returns seg_stats' dict (and "flags", three python ints)."""

    def __init__(self, target: torch.Tensor, K: int, ignore_index: int = -1):
        if target.dim() != 3 or target.shape[1] % 2 or target.shape[2] % 2 or min(target.shape[1:]) < 4:
            raise ValueError(f"PanelStats: target must be [B,H,W] with even H, W >= 4, got {tuple(target.shape)}")
        if int(K) < 1:
            raise ValueError(f"PanelStats: K={K}")
        if not target.is_cuda:
            raise RuntimeError("lseg_hip.metrics.PanelStats runs on the GPU (no CPU fallback): pass CUDA tensors")
        self.lib = _lib.load()
        self.K, self.ignore_index = int(K), int(ignore_index)
        self.target = target.detach().to(torch.int64).contiguous()
        dev, shape = target.device, tuple(target.shape)
        self.label = torch.empty(shape, dtype=torch.int16, device=dev)
        self.best, self.sum, self.tlogit = (torch.empty(shape, dtype=torch.float32, device=dev) for _ in range(3))
        self.next_row = 0

    def fold(self, low: torch.Tensor, row0: int):
        B, H, W = self.target.shape
        if low.dtype != torch.float32 or low.dim() != 4 or (low.shape[0], low.shape[2], low.shape[3]) != (B, H // 2, W // 2) or low.device != self.target.device:
            raise ValueError(f"PanelStats.fold: low must be fp32 [{B}, rows, {H // 2}, {W // 2}] on {self.target.device}, got {tuple(low.shape)} {low.dtype}")
        if int(row0) != self.next_row or row0 + low.shape[1] > self.K:
            raise ValueError(f"PanelStats.fold: panels arrive in ascending order without gaps (expected row0={self.next_row}, got {row0}; K={self.K})")
        low = low.contiguous()
        P = lambda x: C.c_void_p(x.data_ptr())                                     # noqa: E731
        st = torch.cuda.current_stream(low.device).cuda_stream
        _lib.check(self.lib.lseg_op_stats_fold_lowres(P(low), B, low.shape[1], int(row0), H // 2, W // 2, P(self.target), P(self.label), P(self.best),
                                                      P(self.sum), P(self.tlogit), int(row0 == 0), C.c_void_p(st)))
        self.next_row = int(row0) + low.shape[1]

    def finish_device(self):
        """(counts int64 [2+3K], nll float64 [2], flags int64 [3]) on the device, no host synchronisation."""
        if self.next_row != self.K:
            raise RuntimeError(f"PanelStats.finish: {self.next_row} of {self.K} labels were folded")
        B, H, W = self.target.shape
        dev = self.target.device
        counts = torch.empty(2 + 3 * self.K, dtype=torch.int64, device=dev)
        nll = torch.empty(2, dtype=torch.float64, device=dev)
        flags = torch.empty(3, dtype=torch.int64, device=dev)
        nws = int(self.lib.lseg_op_stats_finish_ws_bytes(B, H, W))
        ws = torch.empty(max(nws, 8) // 8, dtype=torch.float64, device=dev)
        P = lambda x: C.c_void_p(x.data_ptr())                                     # noqa: E731
        st = torch.cuda.current_stream(dev).cuda_stream
        _lib.check(self.lib.lseg_op_stats_finish(P(self.label), P(self.best), P(self.sum), P(self.tlogit), P(self.target), B, H, W, self.K,
                                                 self.ignore_index, P(counts), P(nll), P(flags), P(ws), ws.numel() * 8, C.c_void_p(st)))
        return counts, nll, flags

    def finish(self) -> dict:
        counts, nll, flags = self.finish_device()
        n = nll.cpu()
        r = _counts_dict(counts.cpu(), self.K)
        r.update(nll_sum=float(n[0]), nll_count=int(n[1]), flags=[int(f) for f in flags.cpu()])
        return r


def batch_pix_accuracy(output: torch.Tensor, target: torch.Tensor):
    """[3P] encoding.utils.batch_pix_accuracy(output, target) -> (pixel_correct, pixel_labeled)."""
    r = seg_stats(output, target)
    return r["correct"], r["labeled"]


def batch_intersection_union(output: torch.Tensor, target: torch.Tensor, nclass: int):
    """[3P] encoding.utils.batch_intersection_union(output, target, nclass) -> (area_inter, area_union) as numpy int64."""
    if output.shape[1] != nclass:
        raise ValueError(f"output has {output.shape[1]} classes, nclass={nclass}")
    r = seg_stats(output, target)
    return r["area_inter"].numpy(), r["area_union"].numpy()


def cross_entropy(output: torch.Tensor, target: torch.Tensor, ignore_index: int = -1) -> float:
    """Forward value of nn.CrossEntropyLoss(ignore_index=ignore_index)(output, target) (mean over valid pixels)."""
    r = seg_stats(output, target, ignore_index)
    return r["nll_sum"] / r["nll_count"] if r["nll_count"] else float("nan")


class SegmentationMetric:
    """Device-side stand-in for `encoding.utils.SegmentationMetric(nclass)` as test_lseg.py uses it (:319, 385-388):
    `update(labels, preds)`, `get() -> (pixAcc, mIoU)`, `get_all() -> (pixAcc, mIoU, total_inter, total_union)`, `reset()`.
    `preds` are score tensors [B,K,H,W] (or a list of them, like the evaluator's per-image outputs), `labels` the int64
    masks; the per-image statistics come from ONE pass over the scores on the GPU (lseg_op_seg_stats) instead of an
    arg-max + numpy histograms per image on the host.  `all_reduce()` sums the counters over data-parallel ranks."""

    def __init__(self, nclass: int):
        self.nclass = nclass
        self.reset()

    def reset(self):
        self.total_inter = torch.zeros(self.nclass, dtype=torch.int64)
        self.total_union = torch.zeros(self.nclass, dtype=torch.int64)
        self.total_correct = 0
        self.total_label = 0

    def _accumulate(self, correct: int, labeled: int, inter: torch.Tensor, union: torch.Tensor):
        self.total_correct += int(correct)
        self.total_label += int(labeled)
        self.total_inter += inter.to(torch.int64).cpu()
        self.total_union += union.to(torch.int64).cpu()

    def update(self, labels, preds):
        if torch.is_tensor(preds):
            labels, preds = [labels], [preds]
        for label, pred in zip(labels, preds):
            if pred.dim() == 3:
                pred, label = pred.unsqueeze(0), label.unsqueeze(0)
            r = seg_stats(pred, label)
            self._accumulate(r["correct"], r["labeled"], r["area_inter"], r["area_union"])

    def update_labels(self, labels, label_maps):
        """`update` for the routes that give no scores: `label_maps` are predicted label maps ([B,H,W] or [H,W] integer tensors, or a list
        of them -- LSegNet.predict_labels, HipEngine.forward_labels, the `label` plane of BatchedMultiEval.forward_labels) over this
        metric's nclass labels, `labels` the int64 masks.  The same counters as `update` on any scores with that arg-max
        (lseg_op_label_stats)."""
        if torch.is_tensor(label_maps):
            labels, label_maps = [labels], [label_maps]
        if len(labels) != len(label_maps):
            raise ValueError(f"update_labels: {len(labels)} masks for {len(label_maps)} label maps")
        for label, pred in zip(labels, label_maps):
            if pred.dim() == 2:
                pred, label = pred.unsqueeze(0), label.unsqueeze(0)
            r = seg_stats_labels(pred, label.to(pred.device) if torch.is_tensor(label) and pred.is_cuda else label, self.nclass)
            self._accumulate(r["correct"], r["labeled"], r["area_inter"], r["area_union"])

    def all_reduce(self):
        from . import dist as D
        t = torch.cat([torch.tensor([self.total_correct, self.total_label], dtype=torch.int64), self.total_inter, self.total_union])
        t = D.sum_over_ranks(t.cuda() if torch.cuda.is_available() and torch.distributed.is_initialized()
                             and torch.distributed.get_backend() == "nccl" else t).cpu()
        self.total_correct, self.total_label = int(t[0]), int(t[1])
        self.total_inter, self.total_union = t[2:2 + self.nclass].clone(), t[2 + self.nclass:].clone()

    def get_all(self):
        eps = 2.220446049250313e-16                      # np.spacing(1), as in [3P] encoding/utils/metrics.py
        pix_acc = 1.0 * self.total_correct / (eps + self.total_label)
        iou = 1.0 * self.total_inter.double() / (eps + self.total_union.double())
        return pix_acc, float(iou.mean()), self.total_inter.numpy(), self.total_union.numpy()

    def get(self):
        pix_acc, miou, _, _ = self.get_all()
        return pix_acc, miou
