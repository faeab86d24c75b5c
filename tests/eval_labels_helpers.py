"""What the label-panel tests share (tests/test_eval_labels_host.py, tests/test_gpu_eval_labels.py): a numpy restatement of
lseg_op_eval_merge_labels' recurrence -- the state carried from panel to panel as the kernel carries it in memory -- the direct
stable-sort / log-sum-exp reference, and score planes with planted ties."""
import numpy as np
import torch

PARTITIONS = {1: [[1]], 2: [[2], [1, 1]], 5: [[5], [1] * 5, [2, 3]], 37: [[37], [1] * 37, [16, 16, 5]]}


def merge_panel(planes, row0, state, first, last, dtype=np.float64):
    """One call of the kernel: planes [rows, ...] are labels row0 .. in ascending order; state = (label, score, label2, score2, sum) arrays
    or None with first.  `if v > best: runner-up = old best; best = v  elif v > second: second = v`, and the exp-sum relative to the
    running best with one exp per value: exp(-|v - best|) rescales the sum on a new best and is the value's own term otherwise."""
    shape = planes.shape[1:]
    if first:
        lab, lab2 = np.full(shape, -1, np.int16), np.full(shape, -1, np.int16)
        best, sec, s = np.full(shape, -np.inf, dtype), np.full(shape, -np.inf, dtype), np.zeros(shape, dtype)
    else:
        lab, best, lab2, sec, s = (a.copy() for a in state)
    one = dtype(1)
    with np.errstate(invalid="ignore"):
        for j in range(planes.shape[0]):
            v = planes[j].astype(dtype)
            k = np.int16(row0 + j)
            e = np.where(np.isfinite(best), np.exp(-np.abs(v - best), dtype=dtype), dtype(0))
            new = v > best
            s = np.where(new, s * e + one, s + e).astype(dtype)
            run = ~new & (v > sec)
            sec = np.where(new, best, np.where(run, v, sec))
            lab2 = np.where(new, lab, np.where(run, k, lab2)).astype(np.int16)
            best = np.where(new, v, best)
            lab = np.where(new, k, lab).astype(np.int16)
    if last:
        s = (best + np.log(s, dtype=dtype)).astype(dtype)
    return lab, best, lab2, sec, s


def merge_partition(planes, partition, dtype=np.float64):
    """(label, score, label2, score2, lse) of planes [K, ...] (numpy) submitted panel by panel"""
    assert sum(partition) == planes.shape[0]
    state, row0 = None, 0
    for i, rows in enumerate(partition):
        state = merge_panel(planes[row0:row0 + rows], row0, state, i == 0, i == len(partition) - 1, dtype)
        row0 += rows
    return state


def stable_sort_reference(planes):
    """planes: torch [K, ...] -> entries 0 / 1 of the stable descending sort over dim 0 (one label: -1 / -inf) and logsumexp in fp64"""
    val, idx = torch.sort(planes, dim=0, descending=True, stable=True)
    lse = torch.logsumexp(planes.double(), dim=0)
    if planes.shape[0] == 1:
        return idx[0].to(torch.int16), val[0], torch.full_like(idx[0], -1).to(torch.int16), torch.full_like(val[0], float("-inf")), lse
    return idx[0].to(torch.int16), val[0], idx[1].to(torch.int16), val[1], lse


def planted_planes(K, H, W, seed, partition=None):
    """rand * 2 - 1 planes [K, H, W] (torch fp32, CPU) with equal values planted per pixel class (pixel index mod 7): the maximum twice
    inside the first panel (1), across the first panel boundary (2), a LATER plane -- the last -- equal to the winner (3), three equal
    maxima (4), a tied runner-up pair below a single maximum, across the boundary where there is one (5); classes 0 and 6 stay random."""
    g = torch.Generator().manual_seed(seed)
    v = (torch.rand((K, H * W), generator=g) * 2 - 1)
    pix = torch.arange(H * W) % 7
    edge = partition[0] if partition and len(partition) > 1 else max(K // 2, 1)       # first label of the second panel
    top = 1.25

    def put(cls, rows, value):
        m = pix == cls
        for r in rows:
            v[r, m] = value

    if K >= 2:
        put(1, [0, min(edge - 1, K - 1)] if edge >= 2 else [0, 1], top)
        put(2, [edge - 1, min(edge, K - 1)], top)
        m = pix == 3
        v[K - 1, m] = v[:K - 1, m].max(dim=0).values
    if K >= 3:
        put(4, [0, K // 2, K - 1], top)
        put(5, [edge - 1, min(edge + 1, K - 1)] if edge >= 1 and edge + 1 <= K - 1 and edge - 1 != 0 else [1, K - 1], top - 0.5)
        put(5, [0], top)
    return v.view(K, H, W).contiguous()
