"""Multi-scale + flip sliding-window evaluator -- the direct caller of the hot path
(reference: additional_utils/encoding_models.py:54-139 `MultiEvalModule.forward` and
additional_utils/models.py:55-140 `LSeg_MultiEvalModule.forward`).

Same algorithm, same arithmetic order per pixel, but every crop of a scale and its mirrored twin
go through the engine as ONE batch instead of 2 x n_crops separate B=1 forwards (a 4:3 ADE image
costs the reference 36 B=1 forwards, each re-encoding the 150 labels; here 6 batched forwards).
Images of a batch are independent in the engine, so the result is identical to the sequential
schedule.  The data movement around the forwards -- resize / pad / crop / flip / overlap-add / count-normalise -- runs on
the device in three kernels per scale (csrc/evaluator.hip through the C ABI: lseg_op_eval_make_crops / _accumulate /
_resize) when the image lives on the GPU; the torch statement of the same steps below is the definition they are tested
against and what runs for host tensors (tests/test_evaluator_ref_golden.py drives it with a toy module on the CPU).
With lowres=True the forwards stop before the network's x2 output_conv and lseg_op_eval_accumulate_lowres reads the (crop/2, crop/2)
logits through that bilinear on the fly: the same scores bit for bit, a quarter of the logits in memory (DESIGN par. 3.8).
"""
import ctypes as C
import math
from typing import List, NamedTuple, Optional, Sequence, Tuple

import numpy as np
import torch
import torch.nn.functional as F


class ScaleGeometry(NamedTuple):
    """Sizes of one scale: the resized image (height, width), the padded image the sliding window runs over (ph, pw), the crop grid
    (h_grids, w_grids) and the stride."""
    height: int
    width: int
    ph: int
    pw: int
    h_grids: int
    w_grids: int
    stride: int

    @property
    def n_box(self) -> int:
        return self.h_grids * self.w_grids


def scale_geometry(h: int, w: int, scale: float, base_size: int, crop_size: int) -> ScaleGeometry:
    """The sizes of one scale of MultiEvalModule.forward (encoding_models.py:66-99).  One crop when the long side fits."""
    stride = int(crop_size * 2.0 / 3.0)
    long_size = int(math.ceil(base_size * scale))
    if h > w:
        height, width = long_size, int(1.0 * w * long_size / h + 0.5)
    else:
        width, height = long_size, int(1.0 * h * long_size / w + 0.5)
    ph, pw = max(height, crop_size), max(width, crop_size)            # pad_image pads up to the crop size, never beyond
    if long_size <= crop_size:
        h_grids = w_grids = 1
    else:
        h_grids = int(math.ceil(1.0 * (ph - crop_size) / stride)) + 1
        w_grids = int(math.ceil(1.0 * (pw - crop_size) / stride)) + 1
    return ScaleGeometry(height, width, ph, pw, h_grids, w_grids, stride)


def window_partition(n_box: int, max_crops: int, flip: bool):
    """Split the n_box boxes of one scale's grid (row-major (idh, idw) order) into windows [(first_box, n_box), ...] of whole boxes --
    ascending, disjoint, covering -- of at most `max_crops` crops each, a box's mirrored twin (flip) counting with it.  ValueError when
    not even one box (with its twin) fits."""
    per = int(max_crops) // (2 if flip else 1)
    if per < 1:
        raise ValueError(f"max_stack={max_crops} holds no box{' with its mirrored twin' if flip else ''}: it must be at least {2 if flip else 1}")
    return [(first, min(per, n_box - first)) for first in range(0, n_box, per)]


class Step(NamedTuple):
    """One step of the device evaluator's schedule: `scales` (consecutive indices) go through the network as one stack, or -- `windows`
    not None, one scale -- that scale's grid goes through as windows [(first_box, n_box), ...], one forward group each."""
    scales: List[int]
    windows: Optional[List[Tuple[int, int]]] = None


def plan_schedule(geo: Sequence[ScaleGeometry], flip: bool, max_stack: int, max_batch: int) -> Tuple[List[Step], int]:
    """The schedule of one image: (steps, crops of the largest forward group).  EVERY crop of EVERY scale is crop x crop, so consecutive
    scales share a stack while at most `max_stack` crops (mirrored twins included; their [K, crop, crop] fp32 logits are 138 MB per crop
    at K = 150, crop 480 -- a quarter of that with lowres) are alive at once: a 4:3 ADE image (36 crops) is ONE batch-36 forward where a
    forward per scale ran six of 2 .. 12 crops, each at the low-occupancy end of the engine's batch sweep, and a larger image / longer
    scale list runs as several stacks instead of one unbounded allocation (DESIGN par. 3.8).  A scale that alone has more crops than
    max_stack (base 2048 / crop 480 is an 11 x 6 grid at scale 1.75) is a step of its own and runs as windows of whole boxes, each at
    most max_batch crops -- one forward -- where a box and its twin fit in that."""
    twins = 2 if flip else 1
    crops = [twins * g.n_box for g in geo]
    steps, cur, cur_n = [], [], 0
    for i, nc in enumerate(crops):
        if cur and cur_n + nc > max_stack:
            steps.append(Step(cur))
            cur, cur_n = [], 0
        cur.append(i)
        cur_n += nc
    if cur:
        steps.append(Step(cur))
    per_fwd = min(max_stack, max_batch)
    for s, step in enumerate(steps):
        i = step.scales[0]
        if crops[i] > max_stack:             # then the grouping above left it alone
            steps[s] = Step([i], window_partition(geo[i].n_box, per_fwd if per_fwd >= twins else max_stack, flip))
    largest = max(sum(crops[i] for i in st.scales) if st.windows is None else max(twins * nb for _, nb in st.windows) for st in steps)
    return steps, largest


def plan_panels(K: int, panel: int) -> List[Tuple[int, int]]:
    """The label panels [(row0, rows), ...] of a label set of K rows, at most `panel` rows each: ascending, disjoint, covering."""
    K, panel = int(K), int(panel)
    if K < 1 or panel < 1:
        raise ValueError(f"plan_panels: K={K} and panel={panel} must both be at least 1")
    return [(row0, min(panel, K - row0)) for row0 in range(0, K, panel)]


def _pad_image(img, mean, std, crop_size):          # encoding_models.py:144-155
    b, c, h, w = img.shape
    padh = crop_size - h if h < crop_size else 0
    padw = crop_size - w if w < crop_size else 0
    if padh == 0 and padw == 0:
        return img
    pad_values = -np.array(mean) / np.array(std)
    out = img.new_empty((b, c, h + padh, w + padw))
    for i in range(c):
        out[:, i] = F.pad(img[:, i], (0, padw, 0, padh), value=float(pad_values[i]))
    return out


class ModuleSurface(torch.nn.Module):
    """The part of LSegModule's surface the evaluators use (modules/lseg_module.py:29-93: evaluate / evaluate_random, base_size, crop_size,
    mean, std, _up_kwargs) around a bare LSegNet -- for callers that hold a network and no Lightning module (bench.py, tools)."""

    def __init__(self, net, crop_size=480, base_size=520, mean=(0.5, 0.5, 0.5), std=(0.5, 0.5, 0.5)):
        super().__init__()
        self.net, self.crop_size, self.base_size = net, crop_size, base_size
        self.mean, self.std = list(mean), list(std)
        self._up_kwargs = {"mode": "bilinear", "align_corners": True}

    def evaluate(self, x, target=None):
        return self.net(x)

    def evaluate_random(self, x, labelset, target=None):
        return self.net(x, labelset)

    def evaluate_lowres(self, x):
        return self.net.forward_lowres(x)

    def evaluate_random_lowres(self, x, labelset):
        return self.net.forward_lowres(x, labelset)

    def hold_features(self, x):
        return self.net.hold_features(x)

    def score_held(self, held, row0, rows, labelset=""):
        return self.net.score_held(held, row0, rows, labelset)


class BatchedMultiEval(torch.nn.Module):
    """Drop-in for `MultiEvalModule(module, nclass, scales=..., flip=...)` on one GPU.

    `module` needs .evaluate(x) / .evaluate_random(x, labels), .base_size, .crop_size, .mean, .std,
    ._up_kwargs (the LSegModule surface, modules/lseg_module.py:29-93)."""

    def __init__(self, module, nclass, flip=True, scales=(0.5, 0.75, 1.0, 1.25, 1.5, 1.75), max_batch=36, cache_text=True, lowres=False,
                 max_stack=None):
        """max_stack: (device images only) the most crops, mirrored twins included, whose logits are alive at once; None = 48 (192 with
        lowres).  Scales share a forward while they fit; a scale with more crops than that runs as windows of whole boxes through
        lseg_op_eval_accumulate_window(_lowres) + lseg_op_eval_finalize -- the same scores bit for bit (DESIGN par. 3.8).  An attribute
        `max_stack` set on the evaluator afterwards overrides it.
        lowres: (device images only) the forwards stop before the network's output_conv (module.evaluate_lowres /
        evaluate_random_lowres -> fp32 [n, K, crop/2, crop/2]) and lseg_op_eval_accumulate_lowres reads those logits through the x2 bilinear
        on the fly: the same scores bit for bit, a quarter of the logits written, read and alive (DESIGN par. 3.8).  The module must
        offer both *_lowres methods: there is no fallback to the full-resolution path.
        cache_text: encode a label set ONCE per evaluator call chain instead of once per crop batch (the reference re-runs the CLIP text
        tower inside every one of its ~36 forwards per image, lseg_net.py:183 -- the same tokens through the same frozen weights: exact).
        Applied to the wrapped network (`module.net`, an LSegNet) for the duration of a forward and restored afterwards; the engine
        re-encodes whenever the tokens or the weights change (LSegNet._set_tokens / _stamp)."""
        super().__init__()
        self.cache_text = cache_text
        self.module = module
        self.nclass = nclass
        self.base_size = module.base_size
        self.crop_size = module.crop_size
        self.scales = list(scales)
        self.flip = flip
        self.max_batch = max_batch
        self.lowres = bool(lowres)
        self._max_stack = None if max_stack is None else int(max_stack)
        if self.lowres:
            missing = [m for m in ("evaluate_lowres", "evaluate_random_lowres") if not callable(getattr(module, m, None))]
            if missing:
                raise AttributeError(f"BatchedMultiEval(lowres=True) needs module.{' / module.'.join(missing)} "
                                     f"({type(module).__name__} has no such method); there is no fallback to the full-resolution path")
            if self.crop_size % 2 or self.crop_size < 4:
                raise ValueError(f"BatchedMultiEval(lowres=True): crop_size={self.crop_size} must be even and >= 4")

    def _infer(self, crops: torch.Tensor, label_set) -> torch.Tensor:
        """module_inference (encoding_models.py:133-139) for a stack of crops: out = f(x) + flip(f(flip(x)))."""
        xs = torch.cat([crops, torch.flip(crops, dims=[3])], dim=0) if self.flip else crops
        out = self._chunked(xs, label_set, lowres=False)
        if self.flip:
            n = crops.shape[0]
            out = out[:n] + torch.flip(out[n:], dims=[3])
        return out

    @staticmethod
    def _one(img: torch.Tensor) -> torch.Tensor:
        """one image of a list on the device, as forward takes it: float [3,h,w] -> [1,3,h,w]; a decoded uint8 [h,w,3] image as it is"""
        return img.cuda() if img.dtype == torch.uint8 else img.unsqueeze(0).cuda()

    def parallel_forward(self, inputs: Sequence[torch.Tensor], label_set=None) -> List[torch.Tensor]:
        """list of [3,h,w] images in, list of [1,nclass,h,w] score maps out (encoding_models.py:35-52).  Here and in every method below
        an image may also be a decoded one -- torch.uint8 [h,w,3] (HWC, RGB) -- instead of the normalised float tensor: the device kernels
        then apply ToTensor + Normalize(module.mean, module.std) themselves and the results are the same bits."""
        return [self.forward(self._one(img), label_set) for img in inputs]

    def _chunked(self, xs: torch.Tensor, label_set, lowres: bool) -> torch.Tensor:
        """The module's logits of a stack of crops, max_batch crops per forward."""
        suffix = "_lowres" if lowres else ""
        if label_set is None:
            ev = getattr(self.module, "evaluate" + suffix)
        else:
            ev = lambda c: getattr(self.module, "evaluate_random" + suffix)(c, label_set)      # noqa: E731
        outs = [ev(xs[i:i + self.max_batch].contiguous()) for i in range(0, xs.shape[0], self.max_batch)]
        return outs[0] if len(outs) == 1 else torch.cat(outs, dim=0)

    def _module_eval(self, xs: torch.Tensor, label_set) -> torch.Tensor:
        return self._chunked(xs, label_set, self.lowres)

    @staticmethod
    def _image_hw(image: torch.Tensor):
        """(image as the kernels read it, h, w): a normalised float [1,3,h,w] image, or a decoded uint8 [h,w,3] / [1,h,w,3] one"""
        if image.dtype == torch.uint8:
            if image.dim() == 4 and image.shape[0] == 1:
                image = image[0]
            if image.dim() != 3 or image.shape[2] != 3:
                raise ValueError(f"a uint8 image is [h,w,3] (HWC), got {tuple(image.shape)}")
            return image.contiguous(), image.shape[0], image.shape[1]
        batch, ch, h, w = image.shape
        assert batch == 1 and image.dtype == torch.float32
        return image.contiguous(), h, w

    def _scale_crops(self, lib, image, h, w, g, pad, st):
        """The crops (and mirrored twins) of scale geometry g, fp32 [twins * n_box, 3, crop, crop]: resize + make_crops for a float image,
        the one fused kernel (normalise, resize, pad, cut: lseg_op_eval_make_crops_u8, the same bits) for a uint8 one."""
        from . import _lib
        P = lambda t: C.c_void_p(t.data_ptr())       # noqa: E731
        crop, flip = self.crop_size, int(self.flip)
        ch = 3 if image.dtype == torch.uint8 else image.shape[1]
        crops = torch.empty(((2 if self.flip else 1) * g.n_box, ch, crop, crop), dtype=torch.float32, device=image.device)
        if image.dtype == torch.uint8:
            mean, std = ((C.c_float * 3)(*[float(v) for v in m]) for m in (self.module.mean, self.module.std))
            _lib.check(lib.lseg_op_eval_make_crops_u8(P(image), P(crops), h, w, g.height, g.width, crop, g.stride, g.h_grids, g.w_grids, flip,
                                                      pad, mean, std, st))
            return crops
        cur = image.new_empty((ch, g.height, g.width))
        _lib.check(lib.lseg_op_eval_resize(P(image), P(cur), ch, h, w, g.height, g.width, 0, st))
        _lib.check(lib.lseg_op_eval_make_crops(P(cur), P(crops), ch, g.height, g.width, crop, g.stride, g.h_grids, g.w_grids, flip, pad, st))
        return crops

    @torch.no_grad()
    def _forward_device(self, image: torch.Tensor, label_set=None) -> torch.Tensor:
        """The same schedule with the data movement in csrc/evaluator.hip (image on the GPU)."""
        from . import _lib
        lib = _lib.load()
        P = lambda t: C.c_void_p(t.data_ptr())
        st = C.c_void_p(torch.cuda.current_stream(image.device).cuda_stream)
        image, h, w = self._image_hw(image)
        nclass = self.nclass if label_set is None else len(label_set)
        crop = self.crop_size
        if self.module._up_kwargs != {"mode": "bilinear", "align_corners": True}:
            raise ValueError("the device evaluator implements the reference's bilinear / align_corners=True resize")
        pad = (C.c_float * 3)(*[float(v) for v in (-np.array(self.module.mean) / np.array(self.module.std))])
        f32 = torch.empty(0, dtype=torch.float32, device=image.device)         # new_empty / new_zeros of the fp32 maps, whatever the image's dtype
        scores = f32.new_zeros((1, nclass, h, w))
        flip, twins = int(self.flip), 2 if self.flip else 1
        side = crop // 2 if self.lowres else crop
        geo = [scale_geometry(h, w, scale, self.base_size, crop) for scale in self.scales]
        max_stack = getattr(self, "max_stack", None)
        if max_stack is None:
            max_stack = self._max_stack if self._max_stack is not None else (192 if self.lowres else 48)
        steps, largest = plan_schedule(geo, self.flip, int(max_stack), self.max_batch)
        # the largest forward of this call, known before the first: the wrapped network sizes its engine once instead of growing it
        # (closing and rebuilding it) when a later stack is larger than the first
        net = getattr(self.module, "net", None)
        if callable(getattr(net, "reserve_batch", None)):
            net.reserve_batch(min(self.max_batch, largest), crop, crop, None if label_set is None else nclass, image.device)

        def make_crops(g):                   # a scale's crops exist from its step's turn on, not before
            return self._scale_crops(lib, image, h, w, g, pad, st)

        def logits(xs):                      # crops are independent in the engine: the per-crop logits do not depend on the grouping
            outs = self._module_eval(xs, label_set).contiguous()
            assert outs.shape == (xs.shape[0], nclass, side, side) and outs.dtype == torch.float32
            return outs

        def dims(g):                         # the geometry arguments the accumulate and finalize entries share
            return nclass, g.height, g.width, g.ph, g.pw, crop, g.stride, g.h_grids, g.w_grids

        def add_resized(smap, g):            # scores += bilinear(map of the scale)
            _lib.check(lib.lseg_op_eval_resize(P(smap), P(scores), nclass, g.height, g.width, h, w, 1, st))

        accumulate = lib.lseg_op_eval_accumulate_lowres if self.lowres else lib.lseg_op_eval_accumulate
        accumulate_window = lib.lseg_op_eval_accumulate_window_lowres if self.lowres else lib.lseg_op_eval_accumulate_window
        for step in steps:
            stacks = [make_crops(geo[i]) for i in step.scales]
            if step.windows is None:         # one stack: every scale's slice of its logits through the one-launch kernel
                xs = torch.cat(stacks, dim=0) if len(stacks) > 1 else stacks[0]
                outs = logits(xs)
                o0 = 0
                for i in step.scales:
                    g = geo[i]
                    nc = twins * g.n_box
                    smap = f32.new_empty((nclass, g.height, g.width))
                    _lib.check(accumulate(P(outs[o0:o0 + nc]), P(smap), *dims(g), flip, st))     # a contiguous slice: this scale's crops (+ twins)
                    add_resized(smap, g)
                    o0 += nc
                del outs, xs
            else:                            # windows add into the scale's fp32 sum in box order, finalize divides: the same bits
                g, crops = geo[step.scales[0]], stacks[0]
                n = g.n_box
                smap = f32.new_zeros((nclass, g.height, g.width))
                for first, nb in step.windows:
                    xs = torch.cat([crops[first:first + nb], crops[n + first:n + first + nb]], dim=0) if self.flip else crops[first:first + nb]
                    outs = logits(xs)
                    _lib.check(accumulate_window(P(outs), P(smap), *dims(g), flip, first, nb, st))
                    del outs, xs             # one window's logits alive at a time
                _lib.check(lib.lseg_op_eval_finalize(P(smap), P(smap), *dims(g), st))
                add_resized(smap, g)
                del crops
            # nothing of a step stays bound: a name (or a view of the stack) left over keeps its logits alive into the next step's forward
            # (profiles/eval_window.txt: 13 454 MB against 10 553 MB)
            del stacks, smap
        return scores

    @torch.no_grad()
    def forward(self, image: torch.Tensor, label_set=None) -> torch.Tensor:
        if image.is_cuda:
            net = getattr(self.module, "net", None)
            if not self.cache_text or net is None or not hasattr(net, "cache_text"):
                return self._forward_device(image, label_set)
            was = net.cache_text
            net.cache_text = True
            try:
                return self._forward_device(image, label_set)
            finally:
                net.cache_text = was
        return self._forward_torch(image, label_set)

    def parallel_forward_labels(self, inputs: Sequence[torch.Tensor], label_set=None, confidence=False, panel=64) -> List[tuple]:
        """list of [3,h,w] images in, list of forward_labels results out."""
        return [self.forward_labels(self._one(img), label_set, confidence, panel) for img in inputs]

    def parallel_forward_metrics(self, inputs: Sequence[torch.Tensor], targets: Sequence[torch.Tensor], label_set=None, panel=64) -> List[dict]:
        """list of [3,h,w] images and of their [h,w] integer masks in, one dict of pixAcc / IoU counts per image out
        (lseg_hip.metrics.seg_stats_labels of forward_labels' label plane: correct, labeled, area_inter / area_pred / area_lab /
        area_union over the label set) -- the multi-scale masks of a label set of any size scored without any [K,h,w] tensor.  What
        SegmentationMetric.update_labels accumulates from the same planes."""
        from .metrics import seg_stats_labels
        if len(inputs) != len(targets):
            raise ValueError(f"parallel_forward_metrics: {len(inputs)} images for {len(targets)} masks")
        nclass = self.nclass if label_set is None else len(label_set)
        out = []
        for img, tgt in zip(inputs, targets):
            hw = tuple(img.shape[:2]) if img.dtype == torch.uint8 else tuple(img.shape[1:])
            if tuple(tgt.shape) != hw:
                raise ValueError(f"parallel_forward_metrics: a mask of {tuple(tgt.shape)} for an image of {hw}")
            label = self.forward_labels(self._one(img), label_set, False, panel)[0]
            out.append(seg_stats_labels(label.unsqueeze(0), tgt.unsqueeze(0).to(label.device), nclass))
        return out

    @torch.no_grad()
    def forward_labels(self, image: torch.Tensor, label_set=None, confidence=False, panel=64):
        """torch.max(self.forward(image, label_set), 1) for a label set of ANY size without the [K,h,w] score tensor: (label int16 [h,w],
        score fp32 [h,w]); confidence=True adds (label2 int16, score2 fp32, lse fp32) -- entries 0 / 1 of the stable descending sort of the
        scores over the labels and their log-sum-exp.  The multi-scale score is linear in the per-crop logits and those are linear in the
        text rows, so the image tower runs ONCE per crop (module.hold_features keeps what the correlation reads: 15.2 MB per 480^2 crop)
        and the label set is walked in panels of `panel` rows: per panel the held crops are scored (module.score_held), fused by the
        lowres accumulate / finalize / resize kernels with K = rows, and folded into the running per-pixel state by
        lseg_op_eval_merge_labels.  Peak memory follows the panel, not K.  Every evaluator kernel treats planes independently, so a
        plane's fused scores do not depend on the panel that carried it: label / score / label2 / score2 are the same bits for every
        panel size (DESIGN par. 3.8).  Device images only, the lowres arithmetic whatever self.lowres says; the module must offer
        hold_features and score_held: there is no fallback.
        The `label` plane is what lseg_hip.metrics.SegmentationMetric.update_labels (and parallel_forward_metrics above) score against
        a mask: pixAcc / IoU of a label set of any size, without the scores."""
        missing = [m for m in ("hold_features", "score_held") if not callable(getattr(self.module, m, None))]
        if missing:
            raise AttributeError(f"BatchedMultiEval.forward_labels needs module.{' / module.'.join(missing)} "
                                 f"({type(self.module).__name__} has no such method); there is no fallback")
        if not image.is_cuda:
            raise ValueError("BatchedMultiEval.forward_labels runs on device images only")
        if self.crop_size % 2 or self.crop_size < 4:
            raise ValueError(f"BatchedMultiEval.forward_labels: crop_size={self.crop_size} must be even and >= 4")
        net = getattr(self.module, "net", None)
        if net is None or not hasattr(net, "cache_text"):
            return self._forward_labels_device(image, label_set, bool(confidence), int(panel))
        was = net.cache_text
        net.cache_text = True                # the label set is encoded once for the whole call, as in forward
        try:
            return self._forward_labels_device(image, label_set, bool(confidence), int(panel))
        finally:
            net.cache_text = was

    def _forward_labels_device(self, image, label_set, confidence, panel):
        from . import _lib
        lib = _lib.load()
        P = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None
        st = C.c_void_p(torch.cuda.current_stream(image.device).cuda_stream)
        image, h, w = self._image_hw(image)
        f32 = torch.empty(0, dtype=torch.float32, device=image.device)
        nclass = self.nclass if label_set is None else len(label_set)
        panels = plan_panels(nclass, panel)
        crop = self.crop_size
        if self.module._up_kwargs != {"mode": "bilinear", "align_corners": True}:
            raise ValueError("the device evaluator implements the reference's bilinear / align_corners=True resize")
        pad = (C.c_float * 3)(*[float(v) for v in (-np.array(self.module.mean) / np.array(self.module.std))])
        flip, twins = int(self.flip), 2 if self.flip else 1
        side = crop // 2
        geo = [scale_geometry(h, w, scale, self.base_size, crop) for scale in self.scales]
        max_stack = getattr(self, "max_stack", None)
        if max_stack is None:
            max_stack = self._max_stack if self._max_stack is not None else 192
        steps, largest = plan_schedule(geo, self.flip, int(max_stack), self.max_batch)
        net = getattr(self.module, "net", None)
        if callable(getattr(net, "reserve_batch", None)):
            net.reserve_batch(min(self.max_batch, largest), crop, crop, None if label_set is None else nclass, image.device)
        labelset = "" if label_set is None else label_set

        def hold(xs):                        # the towers, once: max_batch crops per forward, what the correlation reads is kept
            return [self.module.hold_features(xs[i:i + self.max_batch].contiguous()) for i in range(0, xs.shape[0], self.max_batch)]

        held = []                            # per step: the held chunks of its stack, or one such list per window
        for step in steps:
            stacks = []
            for i in step.scales:
                stacks.append(self._scale_crops(lib, image, h, w, geo[i], pad, st))
            if step.windows is None:
                held.append(hold(torch.cat(stacks, dim=0) if len(stacks) > 1 else stacks[0]))
            else:
                crops, n = stacks[0], geo[step.scales[0]].n_box
                held.append([hold(torch.cat([crops[first:first + nb], crops[n + first:n + first + nb]], dim=0) if self.flip
                                  else crops[first:first + nb]) for first, nb in step.windows])
            del stacks

        def logits(chunks, row0, rows):      # the panel's planes of a held forward group, [n, rows, crop/2, crop/2]
            outs = [self.module.score_held(hc, row0, rows, labelset) for hc in chunks]
            outs = outs[0] if len(outs) == 1 else torch.cat(outs, dim=0)
            assert outs.shape[1:] == (rows, side, side) and outs.dtype == torch.float32 and outs.is_contiguous()
            return outs

        label = torch.empty((h, w), dtype=torch.int16, device=image.device)
        score = f32.new_empty((h, w))
        label2 = torch.empty_like(label) if confidence else None
        score2, lse = (torch.empty_like(score), torch.empty_like(score)) if confidence else (None, None)
        for pi, (row0, rows) in enumerate(panels):
            scores = f32.new_zeros((rows, h, w))
            for step, hs in zip(steps, held):
                if step.windows is None:
                    outs = logits(hs, row0, rows)
                    o0 = 0
                    for i in step.scales:
                        g = geo[i]
                        nc = twins * g.n_box
                        smap = f32.new_empty((rows, g.height, g.width))
                        _lib.check(lib.lseg_op_eval_accumulate_lowres(P(outs[o0:o0 + nc]), P(smap), rows, g.height, g.width, g.ph, g.pw, crop, g.stride,
                                                                      g.h_grids, g.w_grids, flip, st))
                        _lib.check(lib.lseg_op_eval_resize(P(smap), P(scores), rows, g.height, g.width, h, w, 1, st))
                        o0 += nc
                    del outs, smap
                else:
                    g = geo[step.scales[0]]
                    smap = f32.new_zeros((rows, g.height, g.width))
                    for (first, nb), hw in zip(step.windows, hs):
                        outs = logits(hw, row0, rows)
                        _lib.check(lib.lseg_op_eval_accumulate_window_lowres(P(outs), P(smap), rows, g.height, g.width, g.ph, g.pw, crop, g.stride,
                                                                             g.h_grids, g.w_grids, flip, first, nb, st))
                        del outs
                    _lib.check(lib.lseg_op_eval_finalize(P(smap), P(smap), rows, g.height, g.width, g.ph, g.pw, crop, g.stride, g.h_grids,
                                                         g.w_grids, st))
                    _lib.check(lib.lseg_op_eval_resize(P(smap), P(scores), rows, g.height, g.width, h, w, 1, st))
                    del smap
            _lib.check(lib.lseg_op_eval_merge_labels(P(scores), rows, row0, h, w, P(label), P(score), P(label2), P(score2), P(lse),
                                                     int(pi == 0), int(pi == len(panels) - 1), st))
            del scores
        return (label, score, label2, score2, lse) if confidence else (label, score)

    @torch.no_grad()
    def _forward_torch(self, image: torch.Tensor, label_set=None) -> torch.Tensor:
        """The torch statement of the schedule (host tensors; the definition the device kernels are tested against)."""
        if image.dtype == torch.uint8:
            raise ValueError("a decoded uint8 [h,w,3] image is read by the device kernels only: move it to the GPU (image.cuda()), or "
                             "normalise it to a float [1,3,h,w] tensor for the torch schedule")
        batch, _, h, w = image.shape
        assert batch == 1
        nclass = self.nclass if label_set is None else len(label_set)
        crop_size = self.crop_size
        up = self.module._up_kwargs
        scores = image.new_zeros((batch, nclass, h, w))
        for scale in self.scales:
            height, width, gph, gpw, h_grids, w_grids, stride = scale_geometry(h, w, scale, self.base_size, crop_size)
            long_size, short_size = max(height, width), min(height, width)
            cur_img = F.interpolate(image, (height, width), **up)
            if long_size <= crop_size:
                pad_img = _pad_image(cur_img, self.module.mean, self.module.std, crop_size)
                outputs = self._infer(pad_img, label_set)[:, :, :height, :width]
            else:
                pad_img = _pad_image(cur_img, self.module.mean, self.module.std, crop_size) \
                    if short_size < crop_size else cur_img
                _, _, ph, pw = pad_img.shape
                assert (ph, pw) == (gph, gpw)
                boxes, crops = [], []
                for idh in range(h_grids):
                    for idw in range(w_grids):
                        h0, w0 = idh * stride, idw * stride
                        h1, w1 = min(h0 + crop_size, ph), min(w0 + crop_size, pw)
                        boxes.append((h0, h1, w0, w1))
                        crops.append(_pad_image(pad_img[:, :, h0:h1, w0:w1], self.module.mean, self.module.std,
                                                crop_size))
                outs = self._infer(torch.cat(crops, dim=0), label_set)        # one batched pass per scale
                outputs = image.new_zeros((batch, nclass, ph, pw))
                count_norm = image.new_zeros((batch, 1, ph, pw))
                for k, (h0, h1, w0, w1) in enumerate(boxes):                 # same accumulation order
                    outputs[:, :, h0:h1, w0:w1] += outs[k:k + 1, :, :h1 - h0, :w1 - w0]
                    count_norm[:, :, h0:h1, w0:w1] += 1
                assert (count_norm == 0).sum() == 0
                outputs = (outputs / count_norm)[:, :, :height, :width]
            scores += F.interpolate(outputs, (h, w), **up)
        return scores


class SequentialMultiEval(BatchedMultiEval):
    """The reference's own schedule on the same module: every crop and its mirrored twin as separate B = 1 forwards, each re-encoding the
    label set (encoding_models.py:100-131,133-139), torch ops for the data movement.  What `test_lseg.py` costs per image when nothing is
    batched -- the baseline of bench.py's `eval_multiscale` leg and of the crop-480 parity test; never the default."""

    def __init__(self, module, nclass, flip=True, scales=(0.5, 0.75, 1.0, 1.25, 1.5, 1.75)):
        super().__init__(module, nclass, flip=flip, scales=scales, max_batch=1, cache_text=False)

    def _infer(self, crops, label_set):
        ev = (lambda x: self.module.evaluate(x)) if label_set is None else (lambda x: self.module.evaluate_random(x, label_set))
        outs = []
        for i in range(crops.shape[0]):
            x = crops[i:i + 1].contiguous()
            o = ev(x)
            if self.flip:
                o = o + torch.flip(ev(torch.flip(x, dims=[3]).contiguous()), dims=[3])
            outs.append(o)
        return torch.cat(outs, dim=0)

    @torch.no_grad()
    def forward(self, image, label_set=None):
        return self._forward_torch(image, label_set)
