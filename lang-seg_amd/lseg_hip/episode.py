"""Device-side AverageMeter of the few-shot episode evaluation (the reference's fewshot_data/common/logger.py:10-45).

`EpisodeMeter` holds the per-class intersection / union buffers the reference's AverageMeter holds, as int64 [2, nclass] on the device.
Passed to HipEngine.episode_stats / LSeg.evaluate_episode the kernel scatters every image's areas into column class_id[b] in the same
launch that counts them (csrc/episode.hip: AverageMeter.update's index_add_); `update(inter, union, class_id, loss)` takes explicit
tensors like the reference's.  Nothing synchronises the host until compute_iou().

Differences from the reference, on purpose:
  * the buffers are exact INTEGERS, converted to float32 in compute_iou -- the reference accumulates in float32, which stops counting
    exactly above 2^24 pixels per class (35 images of 480 x 480 of one class reach it);
  * the reference's `assert torch.logical_and(query_ignore_idx, gt_mask).sum() == 0` (evaluation.py:18) would synchronise per batch: the
    kernel counts those pixels (and targets outside {0, 1}) into `flags`, the meter accumulates them, and compute_iou() -- the one
    place that reads back anyway -- raises ValueError when either is non-zero.
"""
from typing import Optional, Sequence, Union

import torch

NCLASS = {"pascal": 20, "coco": 80, "fss": 1000}          # logger.py:17-22


class EpisodeMeter:
    def __init__(self, benchmark: Union[str, int], class_ids_interest: Sequence[int], device=None):
        """benchmark: 'pascal' | 'coco' | 'fss' (nclass 20 / 80 / 1000), or nclass itself; class_ids_interest: dataset.class_ids."""
        if isinstance(benchmark, str):
            if benchmark not in NCLASS:
                raise ValueError(f"unknown benchmark {benchmark!r}: one of {sorted(NCLASS)} or the number of classes")
            self.benchmark, self.nclass = benchmark, NCLASS[benchmark]
        else:
            self.benchmark, self.nclass = None, int(benchmark)
            if self.nclass < 1:
                raise ValueError(f"nclass = {self.nclass}")
        self.device = torch.device(device if device is not None else "cuda")
        ids = [int(c) for c in (class_ids_interest.tolist() if torch.is_tensor(class_ids_interest) else class_ids_interest)]
        if not ids or any(not 0 <= c < self.nclass for c in ids):
            raise ValueError(f"class_ids_interest must be a non-empty subset of [0, {self.nclass})")
        self.class_ids_interest = torch.tensor(ids, dtype=torch.int64, device=self.device)
        self.intersection_buf = torch.zeros((2, self.nclass), dtype=torch.int64, device=self.device)
        self.union_buf = torch.zeros((2, self.nclass), dtype=torch.int64, device=self.device)
        self.flags = torch.zeros(2, dtype=torch.int64, device=self.device)
        self.loss_buf = []                                 # 0-d device tensors, one per update (logger.py:27,34)

    def reset(self):
        self.intersection_buf.zero_()
        self.union_buf.zero_()
        self.flags.zero_()
        self.loss_buf = []

    def note_scatter(self, flags: Optional[torch.Tensor], loss: Optional[torch.Tensor]):
        """The bookkeeping around an update whose index_add_ the kernel already did (HipEngine.episode_stats(meter=...))."""
        if flags is not None:
            self.flags += flags.to(self.device)
        self.loss_buf.append(torch.zeros((), device=self.device) if loss is None else loss.detach().to(self.device))

    def update(self, inter_b: torch.Tensor, union_b: torch.Tensor, class_id, loss: Optional[torch.Tensor] = None,
               flags: Optional[torch.Tensor] = None):
        """AverageMeter.update (logger.py:29-34) on explicit [2, B] areas; duplicate class ids add up (index_add_)."""
        cid = torch.as_tensor(class_id, dtype=torch.int64).to(self.device)
        self.intersection_buf.index_add_(1, cid, inter_b.to(self.device, torch.int64))
        self.union_buf.index_add_(1, cid, union_b.to(self.device, torch.int64))
        self.note_scatter(flags, loss)

    def compute_iou(self):
        """(miou, fb_iou) as logger.py:36-45, float32: IoU = inter / max(union, 1) per class, mIoU = mean over the classes of interest of
        the foreground row x 100, FB-IoU = mean over {background, foreground} of sum(inter) / sum(union) x 100.  Raises ValueError when
        the updates saw ignored pixels with a non-zero target or targets outside {0, 1} (this is where the host reads back)."""
        f = self.flags.tolist()
        if f[0] or f[1]:
            raise ValueError(f"episode meter: {f[0]} pixels are both ignored and labelled (the reference asserts there are none, "
                             f"evaluation.py:18), {f[1]} pixels carry a target outside {{0, 1}}")
        inter, union = self.intersection_buf.float(), self.union_buf.float()
        iou = inter / torch.max(union, torch.ones_like(union))
        iou = iou.index_select(1, self.class_ids_interest)
        miou = iou[1].mean() * 100
        fb_iou = (self.intersection_buf.index_select(1, self.class_ids_interest).sum(dim=1).float()       # summed as integers
                  / self.union_buf.index_select(1, self.class_ids_interest).sum(dim=1).float()).mean() * 100
        return miou, fb_iou
