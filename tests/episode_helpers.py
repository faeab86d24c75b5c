"""Plain-torch restatement of the few-shot episode evaluation, written from its description (not from the reference's text):

  pred = argmax over the 2 label planes (first maximum: a tie is class 0); where the ignore mask is set neither pred nor target counts;
  per image area_pred[c] / area_gt[c] = pixels with pred / target == c (c in {0, 1}; a target outside {0, 1} is in no area_gt and meets
  no prediction), area_inter[c] = pixels with pred == target == c, area_union = area_pred + area_gt - area_inter;
  the meter adds every image's inter / union into column class_id[b] of [2, nclass] buffers; IoU = inter / max(union, 1),
  mIoU = 100 x mean over the classes of interest of the foreground row, FB-IoU = 100 x mean over the two rows of sum(inter) / sum(union);
  the loss is the mean over pixels with target in {0, 1} (and != ignore_index) of logsumexp(v0, v1) - v[target], in fp64.

tests/test_episode_host.py checks it against tests/golden/ref_episode_*.pt (made by the reference's own Evaluator); the GPU tests
use it where the reference cannot go.
"""
import torch


def predict(scores):
    return (scores[:, 1] > scores[:, 0]).long()


def classify(pred, target, ignore=None):
    """areas int64 [B, 6] = {inter0, inter1, pred0, pred1, gt0, gt1} per image."""
    pred, target = pred.long(), target.long()
    B = pred.shape[0]
    on = torch.ones_like(pred, dtype=torch.bool) if ignore is None else (ignore == 0)
    cols = []
    for c in (0, 1):
        cols.append(((pred == c) & (target == c) & on).reshape(B, -1).sum(1))
    for c in (0, 1):
        cols.append(((pred == c) & on).reshape(B, -1).sum(1))
    for c in (0, 1):
        cols.append(((target == c) & on).reshape(B, -1).sum(1))
    return torch.stack(cols, 1)


def inter_union(areas):
    """(area_inter [2, B], area_union [2, B]) in the reference's layout."""
    inter = areas[:, 0:2]
    return inter.t(), (areas[:, 2:4] + areas[:, 4:6] - inter).t()


def flags(target, ignore=None, ignore_index=-100):
    target = target.long()
    f0 = 0 if ignore is None else int(((ignore != 0) & (target != 0)).sum())
    f1 = int(((target != 0) & (target != 1) & (target != ignore_index)).sum())
    return torch.tensor([f0, f1], dtype=torch.int64)


def cross_entropy(scores, target, ignore_index=-100):
    """(sum [B], count [B]) in fp64 of logsumexp(v0, v1) - v[target] over the pixels with target in {0, 1}, != ignore_index."""
    s = scores.double()
    t = target.long()
    B = s.shape[0]
    valid = ((t == 0) | (t == 1)) & (t != ignore_index)
    lse = torch.logsumexp(s, dim=1)
    at = torch.where(t == 1, s[:, 1], s[:, 0])
    nll = torch.where(valid, lse - at, torch.zeros_like(lse))
    return nll.reshape(B, -1).sum(1), valid.reshape(B, -1).sum(1).double()


class Meter:
    """int64 [2, nclass] buffers and the fp64 formulas."""

    def __init__(self, nclass, class_ids_interest):
        self.inter = torch.zeros((2, nclass), dtype=torch.int64)
        self.union = torch.zeros((2, nclass), dtype=torch.int64)
        self.ids = torch.tensor(list(class_ids_interest), dtype=torch.int64)

    def update(self, inter_b, union_b, class_id):
        for b, c in enumerate(int(x) for x in class_id):
            self.inter[:, c] += inter_b[:, b].cpu().long()
            self.union[:, c] += union_b[:, b].cpu().long()

    def compute_iou(self):
        return meter_iou(self.inter, self.union, self.ids)


def meter_iou(inter_buf, union_buf, ids):
    inter, union = inter_buf.cpu().double(), union_buf.cpu().double()
    ids = torch.as_tensor(ids, dtype=torch.int64)
    iou = (inter / union.clamp_min(1.0))[:, ids]
    miou = float(iou[1].mean() * 100)
    fb = float((inter[:, ids].sum(1) / union[:, ids].sum(1)).mean() * 100)
    return miou, fb
