"""Shared pieces of the streamed-loss tests (lseg_op_corr_argmax_loss / lseg_forward_labels_loss): the numpy model of the valid-pixel rule
and of the reduction's partial layout (host tests), the target builder and the guard-banded output set (GPU tests)."""
import ctypes as C

import numpy as np

GUARD = 64
NEG_OTHER = -3                 # a negative target that is never the ignore_index of a case


def valid_mask(target, ignore_index, K):
    """the rule of include/lseg_hip.h (lseg_op_corr_argmax_loss; label_stats.hip pixel_nll): valid iff target != ignore_index and
    0 <= target < K.  K: an int, or one count per image (ragged lists) for a [B, ...] target"""
    t = np.asarray(target)
    k = np.asarray(K).reshape((-1,) + (1,) * (t.ndim - 1)) if np.ndim(K) else K
    return (t != ignore_index) & (t >= 0) & (t < k)


def reduce_model(n, threads, min_pixels, max_groups):
    """cl_plan of csrc/corr_argmax.hip: (pixels per workgroup, workgroups, bytes of partials)"""
    g = min(max(-(-n // min_pixels), 1), max_groups)
    chunk = -(-(-(-n // g)) // threads) * threads
    groups = -(-n // chunk)
    return chunk, groups, groups * 16


def owner_of(n, chunk, threads):
    """(workgroup, lane, step) of every pixel of the flattened maps under the documented layout"""
    i = np.arange(n)
    j = i // chunk
    r = i - j * chunk
    return j, r % threads, r // threads


def nll_model(lse, tlogit, valid, chunk, threads):
    """the reduction in its documented order, in float64: lane sums over ascending steps, the wave's shuffle tree (offsets 32 .. 1), the
    four wave totals ascending, then the fold kernel (lane l: partials l, l + 64, .. ascending; the same tree)"""
    def tree(v):
        v = v.copy()
        for off in (32, 16, 8, 4, 2, 1):
            v[:64 - off] = v[:64 - off] + v[off:64]        # lane i += lane i + off (lanes beyond 64 - off read their own value: unused)
        return v[0]
    d = np.where(valid, lse.astype(np.float64) - tlogit.astype(np.float64), 0.0).ravel()
    n = d.size
    groups = -(-n // chunk)
    partial = np.zeros(groups)
    for j in range(groups):
        blk = d[j * chunk:min((j + 1) * chunk, n)]
        lanes = np.zeros(threads)
        for m in range(0, blk.size, threads):
            seg = blk[m:m + threads]
            lanes[:seg.size] += seg
        waves = [tree(lanes[w * 64:(w + 1) * 64]) for w in range(threads // 64)]
        s = waves[0]
        for w in waves[1:]:
            s += w
        partial[j] = s
    lanes = np.zeros(64)
    for i in range(groups):
        lanes[i % 64] += partial[i]
    return tree(lanes)


def make_target(label0, K, ignore_index, seed):
    """int64 [B, Ho, Wo] in [0, K) at random, with one output row each of: ignore_index, values >= K (K and K + 7), a negative value that
    is not ignore_index, the winner's own label, label 0, label K - 1.  label0: the arg-max of the case (a torch tensor, any device)"""
    import torch
    gen = torch.Generator().manual_seed(seed)
    B, Ho, Wo = label0.shape
    t = torch.randint(0, K, (B, Ho, Wo), generator=gen, dtype=torch.int64)
    t[:, 0] = ignore_index
    t[:, 1, 0::2] = K
    t[:, 1, 1::2] = K + 7
    t[:, 2] = NEG_OTHER if ignore_index != NEG_OTHER else NEG_OTHER - 1
    t[:, 3] = label0[:, 3].long().cpu()
    t[:, 4] = 0
    t[:, 5] = K - 1
    t[:, Ho - 1, Wo - 1] = ignore_index                     # the last pixel of every image too
    return t


class LossOutputs:
    """the outputs of lseg_op_corr_argmax_loss with NaN / -7 guard bands around each; `want` picks the optional ones"""
    NAMES = ("label", "score", "lse", "tlogit", "nll_plane", "nll")

    def __init__(self, B, H, W, want=NAMES):
        import torch
        self.n, self.shape = B * 16 * H * W, (B, 4 * H, 4 * W)
        self.buf = {}
        for k in want:
            if k == "label":
                self.buf[k] = torch.full((self.n + 2 * GUARD,), -7, dtype=torch.int16).cuda()
            elif k == "nll":
                self.buf[k] = torch.full((2 + 2 * GUARD,), float("nan"), dtype=torch.float64).cuda()
            else:
                self.buf[k] = torch.full((self.n + 2 * GUARD,), float("nan")).cuda()

    def ptr(self, k):
        return C.c_void_p(self.buf[k][GUARD:].data_ptr()) if k in self.buf else None

    def ptrs(self):
        return [self.ptr(k) for k in self.NAMES]

    def get(self, k):
        if k == "nll":
            return self.buf[k][GUARD:GUARD + 2]
        return self.buf[k][GUARD:GUARD + self.n].view(self.shape)

    def untouched(self):
        import torch
        return all(((b == -7).all() if k == "label" else torch.isnan(b).all()).item() for k, b in self.buf.items())

    def check_guards(self):
        import torch
        for k, b in self.buf.items():
            ok = (lambda t: (t == -7).all()) if k == "label" else (lambda t: torch.isnan(t).all())
            assert ok(b[:GUARD]) and ok(b[-GUARD:]), f"{k}: written outside the output"
            if k != "label":
                assert not torch.isnan(self.get(k)).any(), f"{k}: an output element was not written"
