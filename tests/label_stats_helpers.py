"""Shared references of the label-statistics tests (tests/test_label_stats_host.py, tests/test_gpu_label_stats.py).

ref_label_stats   the counters of lseg_op_label_stats in numpy (np.bincount): one shared label set, ragged per-image lists, ragged lists
                  mapped into one vocabulary.  `variant` switches in one WRONG rule at a time, for the tests that show the reference
                  tells them apart.
emu_up2           output_conv's x2 bilinear (align_corners=True) with the kernels' fp32 arithmetic (src_tap / bilerp of csrc/common.h)
                  restated on the CPU: the values lseg_op_upsample2x_planes writes, for the widths it does not take (W % 4 != 0).
ref_panel_state   the per-pixel state lseg_op_stats_fold_lowres keeps, in float64, for any partition of the planes into panels.
nll_bound         the counted fp32 error bound of the kernel's per-pixel NLL (below).
"""
import numpy as np

VARIANTS_COUNTS = ("union_for_pred", "ignored_as_labeled", "map_pred_only")
VARIANTS_STATE = ("ge", "wrong_panel")


def ref_label_stats(labels, target, K=None, ignore_index=-1, group_sizes=None, class_map=None, nclass=None, variant=None):
    """labels / target integer arrays [B,H,W].  -> (counts int64 [2 + 3n], flags int64 [2]); the pixel rule of csrc/label_stats.hip:
    t == -1 or ignore_index: nothing; other t < 0: flags[0], nothing; l outside [0, k): flags[1], nothing; else labeled++, pred[l]++,
    t >= k: flags[0]; t < k: lab[t]++ and (l == t, mapped: ids equal) correct++, inter[l]++."""
    labels = np.asarray(labels).astype(np.int64)
    target = np.asarray(target).astype(np.int64)
    B = labels.shape[0]
    if group_sizes is None:
        sizes, offs, n = [int(K)] * B, [0] * (B + 1), int(K)
    else:
        sizes = [int(g) for g in group_sizes]
        offs = [0] + list(np.cumsum(sizes))
        n = int(offs[-1])
    cmap = None
    if class_map is not None:
        cmap, n = np.asarray(class_map, dtype=np.int64), int(nclass)
    inter, pred, lab = (np.zeros(n, np.int64) for _ in range(3))
    correct = labeled = f0 = f1 = 0

    def bins(idx, b, mapped=True):                       # area bins of local indices idx of image b; -1 = no bin
        if cmap is None:
            return idx + offs[b]
        if not mapped:
            return idx
        ids = cmap[offs[b] + idx]
        return np.where((ids >= 0) & (ids < n), ids, -1)

    def add(arr, bn):
        bn = bn[bn >= 0]
        arr += np.bincount(bn, minlength=n)[:n]

    for b in range(B):
        l, t, k = labels[b].reshape(-1), target[b].reshape(-1), sizes[b]
        unl = (t == -1) | (t == ignore_index)
        if variant == "ignored_as_labeled":
            unl = t == -1
        neg = ~unl & (t < 0)
        badl = ~unl & ~neg & ((l < 0) | (l >= k))
        on = ~unl & ~neg & ~badl
        tin = on & (t < k)
        f0 += int(neg.sum()) + int((on & (t >= k)).sum())
        f1 += int(badl.sum())
        labeled += int(on.sum())
        pb = bins(l[on], b)
        tb = bins(t[tin], b, mapped=variant != "map_pred_only")
        add(pred, pb)
        add(lab, tb)
        pbt = bins(l[tin], b)
        hit = (pbt == tb) & (pbt >= 0)
        correct += int(hit.sum())
        add(inter, pbt[hit])
    if variant == "union_for_pred":
        pred = pred + lab - inter
    return np.concatenate([[correct, labeled], inter, pred, lab]).astype(np.int64), np.array([f0, f1], np.int64)


# ---- the x2 bilinear with the kernels' fp32 arithmetic -----------------------------------------------------------------------------------
def _taps(n):
    """src_tap of csrc/common.h for every output index of an axis n -> 2n: s = r * i ROUNDED to fp32, i0 = int(s), l = s - i0."""
    r = np.float32(n - 1) / np.float32(2 * n - 1)
    i = np.arange(2 * n, dtype=np.float32)
    s = (r * i).astype(np.float32)
    i0 = s.astype(np.int64)
    i1 = i0 + (i0 < n - 1)
    return i0, i1, (s - i0.astype(np.float32)).astype(np.float32)


def _fma(a, b, c):
    """fp32 fma: the product of two fp32 is exact in float64; one rounding of the float64 sum on the way back (a double rounding is
    possible in principle, 2^-29 per operation; the GPU test compares this emulation with lseg_op_upsample2x_planes where that runs)."""
    return (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(np.float32)


def emu_up2(planes):
    """planes fp32 [..., h, w] -> [..., 2h, 2w]: bilerp(a, b, c, d, lx, ly) = fma(ly, h1, (1 - ly) * h0), h = fma(lx, b, (1 - lx) * a)."""
    v = np.asarray(planes, dtype=np.float32)
    h, w = v.shape[-2:]
    y0, y1, ly = _taps(h)
    x0, x1, lx = _taps(w)
    one = np.float32(1)
    wx, wy = (one - lx).astype(np.float32), (one - ly).astype(np.float32)
    top, bot = v[..., y0, :], v[..., y1, :]
    h0 = _fma(lx, top[..., x1], (wx * top[..., x0]).astype(np.float32))
    h1 = _fma(lx, bot[..., x1], (wx * bot[..., x0]).astype(np.float32))
    lyc, wyc = ly[:, None], wy[:, None]
    return _fma(np.broadcast_to(lyc, h0.shape), h1, (wyc * h0).astype(np.float32))


# ---- the panel state ------------------------------------------------------------------------------------------------------------------------
def ref_panel_state(up, target, partition, variant=None):
    """up fp32 [B,K,H,W] (the upsampled values), target int [B,H,W], partition = panel sizes summing to K.  -> label int16, best / sum /
    tlogit float64 [B,H,W]: strict `>` keeps the first maximum, sum = sum of exp(v - best) relative to the running best (a new best
    rescales), tlogit = the value of the target's label (NaN where no panel held it)."""
    up = np.asarray(up, dtype=np.float64)
    target = np.asarray(target)
    B, K, H, W = up.shape
    assert sum(partition) == K
    label = np.full((B, H, W), -1, np.int16)
    best = np.full((B, H, W), -np.inf)
    s = np.zeros((B, H, W))
    tl = np.full((B, H, W), np.nan)
    row0 = 0
    for rows in partition:
        for j in range(rows):
            k = row0 + j
            v = up[:, k]
            new = v >= best if variant == "ge" else v > best
            with np.errstate(invalid="ignore"):
                ex = np.exp(-np.abs(v - best))
            s = np.where(new, s * ex + 1.0, s + ex)
            best = np.where(new, v, best)
            label = np.where(new, np.int16(k), label)
            hit = target == (k + rows if variant == "wrong_panel" and k + rows < K else k)
            tl = np.where(hit, v, tl)
        row0 += rows
    return label, best, s, tl


def ref_nll(up, target, ignore_index=-1):
    """float64 {sum, pixels} of logsumexp(up) - up[target] over the valid pixels, and the per-pixel terms the bound needs."""
    up = np.asarray(up, dtype=np.float64)
    B, K, H, W = up.shape
    t = np.asarray(target).astype(np.int64)
    valid = (t != ignore_index) & (t >= 0) & (t < K)
    m = up.max(axis=1)
    lse = m + np.log(np.exp(up - m[:, None]).sum(axis=1))
    at = np.take_along_axis(up, np.clip(t, 0, K - 1)[:, None], axis=1)[:, 0]
    px = lse - at
    return float(px[valid].sum()), int(valid.sum()), m, px, valid


# The kernel's per-pixel NLL is best + log(s) - tlogit in fp32 (u = 2^-24, the unit roundoff), s built over the K labels in order:
#   per label one subtraction v - best (relative u on d: moves exp(-|d|) by |d| exp(-|d|) u <= 0.37 u), one exp2-based exponential
#     (x * log2(e) rounded: relative |d| u on the result, again <= 0.37 u absolute; the hardware exp2: 1 ulp = 2 u relative, <= 2 u
#     absolute since the term is <= 1) and at most a multiplication and an addition into s (2 u relative to s).  s >= 1 always (the running
#     best holds a term 1), so absolute errors of the terms are relative errors of s or less: <= (0.37 + 0.37 + 2 + 2) u < 6 u per label,
#     6 K u on s, hence 6 K u on log(s) to first order
#   log(s) = log2(s) * ln 2: the hardware log2 at 1 ulp and the multiplication, <= 4 u max(1, ln K) absolute (s <= K)
#   best + log(s): one rounding, u (|best| + ln K);  - tlogit: one rounding, u |nll|  (bounded by the former plus |tlogit| <= ... we
#     take 2 u (|best| + ln K) + u |nll| for the pair)
# The float64 accumulation over the pixels adds nothing visible.  Per valid pixel:
U32 = 2.0 ** -24


def nll_bound(K, best64, px64, valid):
    """Sum over the valid pixels of u (6 K + 4 max(1, ln K) + 2 (|best| + ln K) + |nll|): the bound on |kernel nll_sum - float64 nll_sum|."""
    lnk = np.log(max(K, 1))
    per = U32 * (6.0 * K + 4.0 * max(1.0, lnk) + 2.0 * (np.abs(best64) + lnk) + np.abs(px64))
    return float(per[valid].sum())


# ---- inputs ---------------------------------------------------------------------------------------------------------------------------------
def random_case(B, H, W, sizes, seed, ignore_index=255, bad_labels=False):
    """labels within each image's list, targets holding -1, ignore_index, out-of-range values (>= k, and a negative one), and the last
    label; sizes = per-image label counts."""
    g = np.random.default_rng(seed)
    labels = np.stack([g.integers(0, k, size=(H, W)) for k in sizes]).astype(np.int16)
    target = np.stack([g.integers(0, k, size=(H, W)) for k in sizes]).astype(np.int64)
    same = g.random((B, H, W)) < 0.5                           # half the pixels correct
    target = np.where(same, labels.astype(np.int64), target)
    flat = target.reshape(B, -1)
    n = flat.shape[1]
    for b, k in enumerate(sizes):
        special = [-1, ignore_index, k, k + 7, -5, k - 1]
        for i, v in enumerate(special):
            flat[b, (i * 3 + b) % n::max(n // 3, 7)] = v
        if n >= 6:
            flat[b, :6] = special
    if bad_labels and H * W >= 8:
        labels.reshape(B, -1)[:, 7] = np.int16(max(sizes) + 3)
        labels.reshape(B, -1)[:, 6] = -2
    return labels, target


def fold_planes(B, K, h, w, kind, seed, partition):
    """low-resolution planes fp32 [B,K,h,w]: "rand" with exact ties planted across the first panel boundary and a last plane equal to the
    winner, "ramp" ascending from -80 to +80 over the labels (every plane a new best: every step rescales the sum), "flat" all equal."""
    g = np.random.default_rng(seed)
    if kind == "flat":
        return np.full((B, K, h, w), 0.625, np.float32)
    if kind == "ramp":
        lv = np.linspace(-80.0, 80.0, K, dtype=np.float32) if K > 1 else np.array([80.0], np.float32)
        return (lv[None, :, None, None] + g.random((B, 1, h, w), dtype=np.float32) * 0.25).astype(np.float32)
    v = (g.random((B, K, h, w), dtype=np.float32) * 2 - 1).astype(np.float32)
    if K >= 2:
        edge = min(partition[0], K - 1)                        # the first label of the second panel (or the last label)
        v[0, edge] = v[0, edge - 1]                            # image 0: the two planes are equal everywhere, so are their interpolated values,
        v[0, edge - 1:edge + 1, :(h + 1) // 2] += np.float32(2)  # and in the upper half they are the maximum: the lower label must win
        v[:, K - 1, :, ::2] = np.maximum(v[:, K - 1, :, ::2], v.max(axis=1)[:, :, ::2])
    return v


def fold_targets(B, K, H, W, partition, seed):
    """targets on the panel edges (row0, row0 + rows - 1, 0, K - 1), -1, and random labels elsewhere"""
    g = np.random.default_rng(seed)
    t = g.integers(0, K, size=(B, H, W)).astype(np.int64)
    edges, row0 = [0, K - 1, -1], 0
    for rows in partition:
        edges += [row0, row0 + rows - 1]
        row0 += rows
    flat = t.reshape(B, -1)
    for i, e in enumerate(edges):
        flat[:, i::len(edges) + 3] = e
    return t


def partition_of(K, panel):
    return [min(panel, K - r) for r in range(0, K, panel)]
