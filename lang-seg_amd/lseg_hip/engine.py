"""Host-side driver of the HIP engine: owns one C handle per device and feeds it torch
tensors (PyTorch is only the container for HBM allocations and the stream).

Mirrors what `LSeg.forward` (modules/models/lseg_net.py:160-205) needs from the
device side: parameters under the reference's state-dict keys, int64 CLIP tokens,
an fp32 NCHW image batch in, fp32 [B,K,H,W] logits out.
"""
import ctypes as C
from typing import Dict, Iterable, List, Optional, Sequence

import torch

from . import _lib
from .config import LSegConfig

_DT = {torch.float32: _lib.LSEG_F32, torch.float16: _lib.LSEG_F16, torch.bfloat16: _lib.LSEG_BF16,
       torch.int64: _lib.LSEG_I64}
_ACT = {"relu": 0, "lrelu": 1, "tanh": 2}
_RS = {"id": _lib.RS_IDENTITY, "convT": _lib.RS_CONVT, "conv_s2": _lib.RS_CONV_S2}

# state-dict prefixes the engine consumes (everything else, e.g. clip_pretrained.visual.*,
# pretrained.model.norm/head, num_batches_tracked, is host-only baggage)
_SKIP_SUFFIX = ("num_batches_tracked",)
_SKIP_PREFIX = ("clip_pretrained.visual.", "clip_pretrained.logit_scale", "pretrained.model.norm.",
                "pretrained.model.head.")


def _stream_ptr(device) -> int:
    return torch.cuda.current_stream(device).cuda_stream


class _HipMemcpy:
    """device-to-device hipMemcpyAsync by raw pointer (engine-owned memory: BatchNorm sums, momentum buffers)."""
    _hip = None

    @classmethod
    def copy(cls, dst: int, src: int, nbytes: int, stream: int):
        if cls._hip is None:
            cls._hip = C.CDLL("libamdhip64.so")
            cls._hip.hipMemcpyAsync.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p]
            cls._hip.hipMemcpyAsync.restype = C.c_int
        rc = cls._hip.hipMemcpyAsync(C.c_void_p(dst), C.c_void_p(src), nbytes, 3, C.c_void_p(stream))
        if rc != 0:
            raise RuntimeError(f"hipMemcpyAsync failed with {rc}")


def to_c_config(cfg: LSegConfig, img_h: int, img_w: int, max_batch: int, max_labels: int,
                image_dtype: str = "bf16", full_text_context: bool = False, exact_head_grad: bool = False,
                batch_invariant: bool = False, deterministic: bool = False, head_block_training: bool = False,
                train_resnet_decoder: bool = False) -> _lib.LSegConfigC:
    c = _lib.LSegConfigC()
    c.abi_version = _lib.ABI_VERSION
    c.patch, c.dim, c.depth, c.heads = cfg.patch, cfg.dim, cfg.depth, cfg.heads
    for i in range(4):
        c.hooks[i] = cfg.hooks[i]
        c.reassemble_ch[i] = cfg.reassemble[i]
        c.resample_kind[i] = _RS[cfg.resample[i][0]]
        c.resample_k[i] = cfg.resample[i][1]
    c.pos_grid = cfg.pos_grid
    c.features, c.out_c = cfg.features, cfg.out_c
    c.arch_option, c.block_depth = cfg.arch_option, cfg.block_depth
    c.activation = _ACT[cfg.activation]
    t = cfg.text
    c.text_vocab, c.text_ctx, c.text_width, c.text_heads, c.text_layers = t.vocab, t.ctx, t.width, t.heads, t.layers
    c.img_h, c.img_w = img_h, img_w
    c.max_batch, c.max_labels = max_batch, max_labels
    # "strict": split-precision validation mode ((hi, lo) fp16 operand pairs, ~21 mantissa bits; include/lseg_hip.h)
    c.image_dtype = {"bf16": _lib.LSEG_BF16, "fp16": _lib.LSEG_F16, "strict": _lib.LSEG_F16_SPLIT}[image_dtype]
    c.flags = ((1 if full_text_context else 0) | (2 if exact_head_grad else 0) | (4 if batch_invariant else 0)
               | (8 if deterministic else 0) | (16 if head_block_training else 0)
               | (32 if cfg.tower == "resnet101" else 0)           # torchvision ResNet-101 image tower (the ViT fields are ignored)
               | (64 if train_resnet_decoder else 0))              # train the decoder above that tower (lseg_set_train is accepted)
    return c


def check_group_sizes(group_sizes, max_labels: int) -> List[int]:
    """The host-side checks of ragged per-image label lists (set_tokens(group_sizes=...), LSegNet.forward_loss with a list of lists):
    at least one list, every list non-empty, and no more labels than the engine was planned for -- each list and their sum, since the
    lists' text rows are concatenated in the max_labels rows of the text workspace.  Returns the sizes as ints.
    (These are what lseg_set_text_groups refuses as LSEG_ERR_INVALID; since the training step takes the lists they are refused here, as a
    ValueError before the C call, on the inference path of set_tokens / set_text_features as well.)"""
    sizes = [int(k) for k in group_sizes]
    if not sizes:
        raise ValueError("group_sizes is empty: ragged per-image label sets need one list per image")
    for b, k in enumerate(sizes):
        if k < 1:
            raise ValueError(f"group_sizes {sizes}: image {b} has {k} labels; every image needs >= 1 label")
        if k > max_labels:
            raise ValueError(f"group_sizes {sizes}: image {b} has {k} labels > max_labels={max_labels}")
    if sum(sizes) > max_labels:
        raise ValueError(f"group_sizes {sizes}: {sum(sizes)} labels in all > max_labels={max_labels}")
    return sizes


def check_ragged_target(target, B: int, H: int, W: int):
    """The target of the ragged training step: int64 [B, H, W] (image b's values index its own list)."""
    if not torch.is_tensor(target) or target.dtype != torch.int64:
        raise ValueError(f"ragged training target must be an int64 tensor, got {getattr(target, 'dtype', type(target))}")
    if tuple(target.shape) != (B, H, W):
        raise ValueError(f"ragged training target must be [B,H,W] = {(B, H, W)}, got {tuple(target.shape)}")


def image_dims(x: torch.Tensor):
    """(B, H, W) of an image batch in either input format: normalised float [B,3,H,W], or decoded uint8 [B,H,W,3] (set_input_u8)"""
    return (x.shape[0], x.shape[1], x.shape[2]) if x.dtype == torch.uint8 else (x.shape[0], x.shape[2], x.shape[3])


class HipEngine:
    """One engine = one (backbone, H, W, max_batch, max_labels) plan on one GPU."""

    def __init__(self, cfg: LSegConfig, img_h: int, img_w: int, max_batch: int, max_labels: int,
                 device: Optional[torch.device] = None, image_dtype: str = "bf16",
                 full_text_context: bool = False, exact_head_grad: bool = False, batch_invariant: bool = False,
                 deterministic: Optional[bool] = None, head_block_training: bool = False, train_resnet_decoder: bool = False):
        """deterministic: the training step's column sums (bias gradients, BatchNorm batch statistics) in a fixed order instead of
        fp32 atomics -- the same step twice gives bit-identical gradients (include/lseg_hip.h, flags bit 3).  None = the environment's
        LSEG_DETERMINISTIC, default ON: it costs nothing measurable (tools/train_bench.py, B = 8, two interleaved rounds: 41.0 / 41.2 ms
        with it, 41.2 / 41.2 ms on the atomics -- profiles/r05_train_bench.txt); LSEG_DETERMINISTIC=0 / deterministic=False = atomics.
        head_block_training: let set_train(True) accept arch_option 1/2 and train the head blocks (flags bit 4); it costs
        max(block_depth - 1, 0) + 1 saved fp32 [max_batch, max_labels, h, w] plane sets.
        train_resnet_decoder: on a ResNet-101 tower config (clip_resnet101), let set_train(True) / enable_training train the decoder
        above the tower (flags bit 6): the tower runs in train() mode -- batch-statistics BatchNorm, running buffers updated in the bound
        tensors -- and gets no gradient; scratch.* is the trainable set.  On a ViT config the engine refuses it (LSEG_ERR_INVALID)."""
        import os
        if deterministic is None:
            deterministic = os.environ.get("LSEG_DETERMINISTIC", "1") not in ("", "0")
        self.deterministic = bool(deterministic)
        self.lib = _lib.load()
        if not torch.cuda.is_available():
            raise _lib.LSegError(-2, "no GPU visible: the LSeg HIP engine has no CPU fallback")
        self.device = torch.device(device if device is not None else f"cuda:{torch.cuda.current_device()}")
        self.cfg = cfg
        self.img_h, self.img_w = img_h, img_w
        self.max_batch, self.max_labels = max_batch, max_labels
        self._c = to_c_config(cfg, img_h, img_w, max_batch, max_labels, image_dtype, full_text_context, exact_head_grad, batch_invariant,
                               self.deterministic, head_block_training, train_resnet_decoder)
        self.train_resnet_decoder = bool(train_resnet_decoder)
        h = C.c_void_p()
        _lib.check(self.lib.lseg_create(C.byref(self._c), self.device.index or 0, C.byref(h)))
        self._h = h
        self._K = 0
        self._group = 0
        self._groups: Optional[List[int]] = None           # ragged per-image label sets (lseg_set_text_groups)
        self._keep: List[torch.Tensor] = []
        self.training = False
        self.image_dtype = image_dtype
        self.grads: Dict[str, torch.Tensor] = {}
        self.frozen_encoder = False
        self.input_u8 = None                               # (mean, std) while the uint8 input format is set (set_input_u8)
        self._cb_error: Optional[BaseException] = None     # first exception raised inside a ctypes callback (ctypes would swallow it)

    def close(self):
        if getattr(self, "_h", None):
            self.lib.lseg_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ---- parameters -------------------------------------------------------------------------------
    def load_state_dict(self, sd: Dict[str, torch.Tensor], prefix: str = ""):
        """Bind every tensor of a (reference-layout) state dict and repack on the device.  Tensors already on the engine's device
        are bound IN PLACE (no copy): they are the fp32 masters the fused SGD step updates and the BatchNorm running statistics
        train mode writes (include/lseg_hip.h); `self.bound[key]` is the device tensor behind each key."""
        st = _stream_ptr(self.device)
        self.bound: Dict[str, torch.Tensor] = {}
        for k, v in sd.items():
            if prefix:
                if not k.startswith(prefix):
                    continue
                k = k[len(prefix):]
            if k.endswith(_SKIP_SUFFIX) or k.startswith(_SKIP_PREFIX):
                continue
            if v.dtype not in _DT:
                continue
            t = v.detach().to(self.device).contiguous()
            self.bound[k] = t
            shape = (C.c_int64 * max(1, t.dim()))(*t.shape)
            _lib.check(self.lib.lseg_bind_param(self._h, k.encode(), C.c_void_p(t.data_ptr()), _DT[t.dtype],
                                                shape, t.dim()))
        _lib.check(self.lib.lseg_finalize_params(self._h, C.c_void_p(st)))

    # ---- text -------------------------------------------------------------------------------------------
    def set_tokens(self, tokens: torch.Tensor, labels_per_image: int = 0, group_sizes: Optional[Sequence[int]] = None):
        """tokens int64 [K, ctx].  labels_per_image = k > 0 (LSegNetZS, lseg_net_zs.py:177-214): the K = B*k rows are
        per-image label sets, image b is correlated with rows [b*k, (b+1)*k) and forward returns [B, k, H, W].
        group_sizes = [k_0, .., k_{B-1}] (lseg_set_text_groups): ragged per-image label sets -- image b owns k_b consecutive rows of the
        K = sum(k_b); forward_labels / forward_labels_conf then return labels indexing each image's own list, every other inference forward
        raises.  While training, forward(x, want_logits=False) + train_loss / backward(target=...) take them: the target of image b holds
        values in [0, k_b) or ignore_index (the fused-loss route; there are no [B,K,H,W] logits and no d(logits) hand-over)."""
        if group_sizes is not None and labels_per_image:
            raise ValueError("labels_per_image and group_sizes are two different groupings: give one")
        tok = tokens.detach().to("cpu", torch.int64).contiguous()
        K, ctx = tok.shape
        arr = (C.c_int64 * (K * ctx)).from_buffer_copy(tok.numpy().tobytes())
        _lib.check(self.lib.lseg_set_text_tokens(self._h, arr, K, ctx))
        _lib.check(self.lib.lseg_set_text_grouping(self._h, int(labels_per_image)))
        self._K = K
        self._group = int(labels_per_image)
        self._set_groups(group_sizes)

    def _set_groups(self, group_sizes: Optional[Sequence[int]]):
        self._groups = None
        if group_sizes is None:
            _lib.check(self.lib.lseg_set_text_groups(self._h, None, 0))
            return
        sizes = check_group_sizes(group_sizes, self.max_labels)
        if sum(sizes) != self._K:
            raise ValueError(f"group_sizes {sizes} do not add up to the {self._K} text rows")
        _lib.check(self.lib.lseg_set_text_groups(self._h, (C.c_int32 * len(sizes))(*sizes), len(sizes)))
        self._groups = sizes

    def clear_grouping(self):
        """One label set shared by the batch again: drops a per-image grouping of either kind (lseg_set_text_grouping(0) clears both)."""
        _lib.check(self.lib.lseg_set_text_grouping(self._h, 0))
        self._group, self._groups = 0, None

    def set_text_features(self, feat: torch.Tensor, group_sizes: Optional[Sequence[int]] = None):
        """fp16 [K, out_c] text features computed elsewhere (un-normalised `encode_text` output or already normalised): replaces the
        tokens; the engine's text tower is not run until set_tokens is called again (lseg_set_text_features).  group_sizes: as in
        set_tokens (ragged per-image label sets over the K rows)."""
        f = feat.detach().to(self.device, torch.float16).contiguous()
        if f.dim() != 2 or f.shape[1] != self.cfg.out_c:
            raise ValueError(f"text features must be [K, {self.cfg.out_c}], got {tuple(f.shape)}")
        _lib.check(self.lib.lseg_set_text_features(self._h, C.c_void_p(f.data_ptr()), f.shape[0], C.c_void_p(_stream_ptr(self.device))))
        self._keep = [f]
        self._K = f.shape[0]
        if self._group:
            _lib.check(self.lib.lseg_set_text_grouping(self._h, 0))
        self._group = 0
        self._set_groups(group_sizes)

    def encode_text(self) -> torch.Tensor:
        _lib.check(self.lib.lseg_encode_text(self._h, C.c_void_p(_stream_ptr(self.device))))
        out = torch.empty((self._K, self.cfg.out_c), dtype=torch.float16, device=self.device)
        _lib.check(self.lib.lseg_get_text_features(self._h, C.c_void_p(out.data_ptr()),
                                                   C.c_void_p(_stream_ptr(self.device))))
        return out

    def set_text_cache(self, enabled: bool):
        _lib.check(self.lib.lseg_set_text_cache(self._h, int(enabled)))

    # ---- forward -----------------------------------------------------------------------------------------
    def set_input_u8(self, enabled: bool = True, mean=(0.5, 0.5, 0.5), std=(0.5, 0.5, 0.5)):
        """The input format of every forward method (lseg_set_input_u8).  enabled: x is a decoded image batch, uint8 [B,H,W,3] (HWC, RGB,
        contiguous) on the engine's device, and the first stage applies ToTensor + Normalize(mean, std) -- (v / 255 - mean) / std in fp32,
        torch's operations and rounding, so every output equals the one for the tensor that transform gives.  Not enabled (the default
        state): x is the normalised float32 [B,3,H,W] tensor.  LSEG_ERR_INVALID for a std of 0 or a non-finite value, LSEG_ERR_UNSUPPORTED
        on a "strict" engine (its first stage reads fp32 only); the format then stays what it was.
        The kernels read the batch in 16-byte chunks from its first byte: a batch whose storage does not start on a 16-byte boundary (a
        slice such as u8[1:] of a larger batch can) is copied to a fresh allocation by the forward methods; the C entries refuse it."""
        if not enabled:
            _lib.check(self.lib.lseg_set_input_u8(self._h, 0, None, None))
            self.input_u8 = None
            return
        mean, std = [float(v) for v in mean], [float(v) for v in std]
        if len(mean) != 3 or len(std) != 3:
            raise ValueError(f"set_input_u8: mean and std are 3 values each (RGB), got {len(mean)} and {len(std)}")
        _lib.check(self.lib.lseg_set_input_u8(self._h, 1, (C.c_float * 3)(*mean), (C.c_float * 3)(*std)))
        self.input_u8 = (tuple(mean), tuple(std))

    def _check_input(self, x: torch.Tensor):
        """The image batch against the engine's plan and input format.  A batch in the OTHER format than the one set is refused as
        LSegError LSEG_ERR_INVALID (-1): the C entries cannot tell a uint8 pointer from a float one, so it is decided here."""
        if x.dtype == torch.uint8:
            if self.input_u8 is None:
                raise _lib.LSegError(-1, "x is a uint8 image batch but the engine reads float32 [B,3,H,W]: call set_input_u8(True, mean, std) first")
            if x.device != self.device:
                raise ValueError(f"x must live on {self.device}, got {x.device}")
            if x.dim() != 4 or tuple(x.shape[1:]) != (self.img_h, self.img_w, 3):
                raise _lib.LSegError(-1, f"uint8 input is [B,H,W,3] (HWC) = [B,{self.img_h},{self.img_w},3] for this engine, got {tuple(x.shape)}")
        else:
            if self.input_u8 is not None:
                raise _lib.LSegError(-1, f"the engine's input format is uint8 [B,H,W,3] (set_input_u8), got {x.dtype}: call set_input_u8(False) "
                                         "for normalised float32 [B,3,H,W] input")
            if x.device != self.device or x.dtype != torch.float32:
                raise ValueError(f"x must be float32 on {self.device}, got {x.dtype} on {x.device}")
            if x.dim() != 4 or tuple(x.shape[1:]) != (3, self.img_h, self.img_w):
                raise ValueError(f"engine was planned for 3x{self.img_h}x{self.img_w}, got {'x'.join(str(d) for d in x.shape[1:])}")
        x = x.contiguous()
        if x.dtype == torch.uint8 and x.data_ptr() % 16:        # the uint8 first stages load 16-byte chunks (lseg_set_input_u8)
            x = x.clone()
        B = x.shape[0]
        if self._group > 0 and self._K != B * self._group:
            raise ValueError(f"per-image label sets: {self._K} token rows != batch {B} x {self._group}")
        if self._groups is not None and len(self._groups) != B:
            raise ValueError(f"ragged per-image label sets: {len(self._groups)} label lists != batch {B}")
        return x

    def _refuse_ragged(self, x: torch.Tensor):
        """ragged label sets have no logits: the C entry refuses before any kernel runs (LSEG_ERR_UNSUPPORTED), with its own message"""
        if self._groups is not None:
            if self.training:
                raise _lib.LSegError(-5, "ragged per-image label sets have no [B,K,H,W] logits: in train mode call forward(x, want_logits=False) "
                                         "and take the loss from train_loss / backward(target=...)")
            _lib.check(self.lib.lseg_forward(self._h, C.c_void_p(x.data_ptr()), x.shape[0], None, None, C.c_void_p(_stream_ptr(self.device))))
            raise RuntimeError("lseg_forward accepted ragged label sets")

    def forward_labels(self, x: torch.Tensor, want_score: bool = False):
        """Masks for any K <= 32767 (lseg_forward_labels): int16 [B,H,W] = torch.max(logits, 1)[1] of the logits forward() would return,
        without those logits -- and, with want_score, fp32 [B,H,W] = torch.max(logits, 1)[0]."""
        x = self._check_input(x)
        B, H, W = image_dims(x)
        lab = torch.empty((B, H, W), dtype=torch.int16, device=self.device)
        score = torch.empty((B, H, W), dtype=torch.float32, device=self.device) if want_score else None
        _lib.check(self.lib.lseg_forward_labels(
            self._h, C.c_void_p(x.data_ptr()), B, C.c_void_p(lab.data_ptr()),
            C.c_void_p(score.data_ptr()) if score is not None else None, C.c_void_p(_stream_ptr(self.device))))
        self._raise_callback_error()
        return (lab, score) if want_score else lab

    def forward_labels_conf(self, x: torch.Tensor) -> Dict[str, torch.Tensor]:
        """forward_labels with a confidence (lseg_forward_labels_conf), still without the [B,K,H,W] logits: a dict of [B,H,W] tensors --
        "label" int16 / "score" fp32 = torch.max(logits, 1); "label2" int16 / "score2" fp32 = the runner-up, entry 1 of
        torch.sort(logits, 1, descending=True, stable=True) (-1 / -inf with a single label); "lse" fp32 = torch.logsumexp(logits, 1).
        The winner's softmax probability is exp(score - lse), the top-2 margin score - score2."""
        x = self._check_input(x)
        B, H, W = image_dims(x)
        out = {"label": torch.empty((B, H, W), dtype=torch.int16, device=self.device),
               "score": torch.empty((B, H, W), dtype=torch.float32, device=self.device),
               "label2": torch.empty((B, H, W), dtype=torch.int16, device=self.device),
               "score2": torch.empty((B, H, W), dtype=torch.float32, device=self.device),
               "lse": torch.empty((B, H, W), dtype=torch.float32, device=self.device)}
        _lib.check(self.lib.lseg_forward_labels_conf(
            self._h, C.c_void_p(x.data_ptr()), B, *(C.c_void_p(out[k].data_ptr()) for k in ("label", "score", "label2", "score2", "lse")),
            C.c_void_p(_stream_ptr(self.device))))
        self._raise_callback_error()
        return out

    def forward_labels_loss(self, x: torch.Tensor, target: torch.Tensor, ignore_index: int = -1, plane: bool = False) -> Dict[str, torch.Tensor]:
        """forward_labels with the cross-entropy against `target` int64 [B,H,W] (lseg_forward_labels_loss), without the [B,K,H,W] logits,
        for one shared label set of any K or ragged per-image lists (the target of image b then indexes its own list).  A dict of DEVICE
        tensors, no host synchronisation: "label" int16 / "score" / "lse" fp32 [B,H,W] as forward_labels_conf gives them; "nll" float64 [2]
        = {sum over the valid pixels (target != ignore_index and inside the image's label range) of lse - logit[target], their number};
        "counts" int64 = label_stats' counters of "label" against the target ([2 + 3K]; ragged: [2 + 3 sum of the list lengths]); with
        plane=True also "nll_plane" fp32 [B,H,W], the per-pixel loss (0 where the pixel is not valid)."""
        x = self._check_input(x)
        B, H, W = image_dims(x)
        if not torch.is_tensor(target) or tuple(target.shape) != (B, H, W) or target.dtype.is_floating_point:
            raise ValueError(f"forward_labels_loss: target must be an integer tensor [{B},{H},{W}]")
        t = target.detach().to(self.device, torch.int64).contiguous()
        n = sum(self._groups) if self._groups is not None else (self._group if self._group > 0 else self._K)
        out = {"label": torch.empty((B, H, W), dtype=torch.int16, device=self.device),
               "score": torch.empty((B, H, W), dtype=torch.float32, device=self.device),
               "lse": torch.empty((B, H, W), dtype=torch.float32, device=self.device),
               "nll": torch.empty(2, dtype=torch.float64, device=self.device),
               "counts": torch.empty(2 + 3 * n, dtype=torch.int64, device=self.device)}
        if plane:
            out["nll_plane"] = torch.empty((B, H, W), dtype=torch.float32, device=self.device)
        P = lambda k: C.c_void_p(out[k].data_ptr()) if k in out else None       # noqa: E731
        _lib.check(self.lib.lseg_forward_labels_loss(
            self._h, C.c_void_p(x.data_ptr()), B, C.c_void_p(t.data_ptr()), int(ignore_index), P("label"), P("score"), P("lse"), P("nll_plane"),
            P("nll"), P("counts"), C.c_void_p(_stream_ptr(self.device))))
        self._raise_callback_error()
        return out

    def forward_lowres(self, x: torch.Tensor) -> torch.Tensor:
        """fp32 [B,Kout,H/2,W/2]: the logits before output_conv's x2 bilinear (lseg_forward_lowres) -- lseg_op_upsample2x_planes of them is
        bit-identical to forward(x); the [B,Kout,H,W] tensor is never written."""
        x = self._check_input(x)
        self._refuse_ragged(x)
        B, H, W = image_dims(x)
        Kout = self._group if self._group > 0 else self._K
        low = torch.empty((B, Kout, H // 2, W // 2), dtype=torch.float32, device=self.device)
        _lib.check(self.lib.lseg_forward_lowres(self._h, C.c_void_p(x.data_ptr()), B, C.c_void_p(low.data_ptr()),
                                                C.c_void_p(_stream_ptr(self.device))))
        self._raise_callback_error()
        return low

    def forward_features(self, x: torch.Tensor):
        """(feat fp16 [B, H/4+2, W/4+2, out_c], scale fp32 [B, H/2, W/2]): what the correlation reads after the image tower
        (lseg_forward_features) -- held by the caller, any slice of a label set is scored from them later (score_features).  No text is
        read.  Per-image label sets, train mode and the schedules without the commuted correlation raise LSEG_ERR_UNSUPPORTED."""
        x = self._check_input(x)
        B, H, W = image_dims(x)
        fb, sb = C.c_size_t(), C.c_size_t()
        _lib.check(self.lib.lseg_features_bytes(self._h, B, C.byref(fb), C.byref(sb)))
        assert fb.value == B * (H // 4 + 2) * (W // 4 + 2) * self.cfg.out_c * 2 and sb.value == B * (H // 2) * (W // 2) * 4
        feat = torch.empty((B, H // 4 + 2, W // 4 + 2, self.cfg.out_c), dtype=torch.float16, device=self.device)
        scale = torch.empty((B, H // 2, W // 2), dtype=torch.float32, device=self.device)
        _lib.check(self.lib.lseg_forward_features(self._h, C.c_void_p(x.data_ptr()), B, C.c_void_p(feat.data_ptr()), C.c_void_p(scale.data_ptr()),
                                                  C.c_void_p(_stream_ptr(self.device))))
        self._raise_callback_error()
        return feat, scale

    def score_features(self, feat: torch.Tensor, scale: torch.Tensor, row0: int, rows: int) -> torch.Tensor:
        """fp32 [B, rows, H/2, W/2]: the low-resolution logits of text rows [row0, row0 + rows) of the current label set for held features
        (lseg_score_features) -- the planes forward_lowres gives for them (bit for bit where it takes the generic correlation, K > 157)."""
        B = feat.shape[0]
        H, W = self.img_h, self.img_w
        if (feat.dtype != torch.float16 or scale.dtype != torch.float32 or feat.device != self.device or scale.device != self.device
                or tuple(feat.shape) != (B, H // 4 + 2, W // 4 + 2, self.cfg.out_c) or tuple(scale.shape) != (B, H // 2, W // 2)
                or not feat.is_contiguous() or not scale.is_contiguous()):
            raise ValueError(f"held features of another engine plan: feat {tuple(feat.shape)} {feat.dtype}, scale {tuple(scale.shape)} {scale.dtype} "
                             f"for an engine of {H}x{W} on {self.device}")
        low = torch.empty((B, max(int(rows), 0), H // 2, W // 2), dtype=torch.float32, device=self.device)
        _lib.check(self.lib.lseg_score_features(self._h, C.c_void_p(feat.data_ptr()), C.c_void_p(scale.data_ptr()), B, int(row0), int(rows),
                                                C.c_void_p(low.data_ptr()), C.c_void_p(_stream_ptr(self.device))))
        return low

    def forward(self, x: torch.Tensor, want_logits: bool = True, want_argmax: bool = False):
        x = self._check_input(x)
        if not (self._groups is not None and self.training and not want_logits and not want_argmax):    # the ragged training step: loss only
            self._refuse_ragged(x)
        B, H, W = image_dims(x)
        Kout = self._group if self._group > 0 else self._K
        if want_argmax and not want_logits and Kout > 256:
            return self.forward_labels(x)                     # uint8 cannot hold the labels: the int16 masks (uint8 stays the K <= 256 form)
        logits = torch.empty((B, Kout, H, W), dtype=torch.float32, device=self.device) if want_logits else None
        amax = torch.empty((B, H, W), dtype=torch.uint8, device=self.device) if want_argmax else None      # the masks
        _lib.check(self.lib.lseg_forward(
            self._h, C.c_void_p(x.data_ptr()), B,
            C.c_void_p(logits.data_ptr()) if logits is not None else None,
            C.c_void_p(amax.data_ptr()) if amax is not None else None,
            C.c_void_p(_stream_ptr(self.device))))
        self._raise_callback_error()
        if want_logits and want_argmax:
            return logits, amax
        return logits if want_logits else amax

    # ---- training step (include/lseg_hip.h "training step"; modules/lsegmentation_module.py:66-81) ---------------------
    def trainable_keys(self, sd: Dict[str, torch.Tensor]) -> List[str]:
        """State-dict keys (relative to `net.`) the backward produces gradients for, in bucket order."""
        keys = []
        for k, v in sd.items():
            if not v.is_floating_point() or v.dtype != torch.float32 or k.endswith(("running_mean", "running_var")):
                continue
            if k.startswith(_SKIP_PREFIX) or ".refinenet4.resConfUnit1." in k or k.startswith("clip_pretrained."):
                continue
            b = self.lib.lseg_grad_bucket(self._h, k.encode())
            if b >= 0:
                keys.append((b, k))
        return [k for _, k in sorted(keys, key=lambda t: t[0])]

    def set_frozen_encoder(self, enabled: bool = True):
        """pretrained.model.* stops being trainable (lseg_set_frozen_encoder): legal only before the first set_train(True)."""
        _lib.check(self.lib.lseg_set_frozen_encoder(self._h, int(enabled)))
        self.frozen_encoder = bool(enabled)

    def enable_training(self, sd: Dict[str, torch.Tensor], freeze_encoder: bool = False):
        """net.train(): allocate the saved-activation workspace, and one FLAT fp32 gradient buffer per bucket (what the RCCL
        all-reduce runs on, in place); every parameter's gradient is a view into its bucket, bound to the engine.
        freeze_encoder: the clip_fixed setup (lsegmentation_module_zs.py:220-235) without its wasted work -- pretrained.model.* gets no
        gradient (it is absent from `self.grads`), the backward stops at the four readouts, the optimizer steps skip it."""
        if freeze_encoder:
            self.set_frozen_encoder(True)
        _lib.check(self.lib.lseg_set_train(self._h, 1))
        nb = self.lib.lseg_num_grad_buckets(self._h)
        groups: List[List[str]] = [[] for _ in range(nb)]
        for k in self.trainable_keys(sd):
            groups[self.lib.lseg_grad_bucket(self._h, k.encode())].append(k)
        self.grad_buckets: List[torch.Tensor] = []
        self.grads = {}
        for ks in groups:
            n = sum(sd[k].numel() for k in ks)
            flat = torch.zeros(max(n, 1), dtype=torch.float32, device=self.device)
            off = 0
            for k in ks:
                m = sd[k].numel()
                view = flat[off:off + m].view(sd[k].shape)
                _lib.check(self.lib.lseg_bind_grad(self._h, k.encode(), C.c_void_p(view.data_ptr())))
                self.grads[k] = view
                off += m
            self.grad_buckets.append(flat)
        self._loss = torch.zeros(2, dtype=torch.float64, device=self.device)
        self.training = True

    def set_train(self, enabled: bool):
        _lib.check(self.lib.lseg_set_train(self._h, int(enabled)))
        self.training = bool(enabled)

    def _raise_callback_error(self):
        """Exceptions raised inside the bucket / SyncBatchNorm callbacks cannot cross the C frames (ctypes prints and drops them):
        the trampolines park the first one here and it is re-raised as soon as the C call that triggered it has returned."""
        if self._cb_error is not None:
            e, self._cb_error = self._cb_error, None
            raise RuntimeError("a gradient-bucket / SyncBatchNorm callback failed during the engine call; gradients or batch "
                               "statistics of this step are NOT exchanged") from e

    def backward(self, target: Optional[torch.Tensor] = None, dlogits: Optional[torch.Tensor] = None,
                 ignore_index: int = -1, accumulate: bool = False, grad_scale: Optional[torch.Tensor] = None) -> Optional[torch.Tensor]:
        """After a train-mode forward.  target int64 [B,H,W] -> returns the mean cross-entropy (0-dim tensor on the device,
        no host sync); or dlogits fp32 [B,K,H,W] (autograd hand-over) -> None.  Gradients land in self.grads / grad_buckets.
        grad_scale (fp32 0-dim device tensor, target form only): d(loss) of an autograd caller, read by the kernel (lseg_backward_scaled)."""
        st = C.c_void_p(_stream_ptr(self.device))
        if target is not None and self._groups is not None:
            check_ragged_target(target, len(self._groups), self.img_h, self.img_w)
        if dlogits is not None:
            dl = dlogits.contiguous()
            assert dl.dtype == torch.float32 and dl.device == self.device
            _lib.check(self.lib.lseg_backward(self._h, C.c_void_p(dl.data_ptr()), None, ignore_index, int(accumulate), None, st))
            self._raise_callback_error()
            return None
        t = target.contiguous()
        assert t.dtype == torch.int64 and t.device == self.device
        if grad_scale is not None:
            gs = grad_scale.detach().to(self.device, torch.float32).reshape(1).contiguous()
            self._keep = [t, gs]                                  # alive until the kernels that read them have been enqueued AND run
            _lib.check(self.lib.lseg_backward_scaled(self._h, C.c_void_p(t.data_ptr()), ignore_index, int(accumulate),
                                                     C.c_void_p(gs.data_ptr()), st))
            self._raise_callback_error()
            return None
        _lib.check(self.lib.lseg_backward(self._h, None, C.c_void_p(t.data_ptr()), ignore_index, int(accumulate),
                                          C.c_void_p(self._loss.data_ptr()), st))
        self._raise_callback_error()
        return (self._loss[0] / self._loss[1]).float()

    def train_loss(self, target: torch.Tensor, ignore_index: int = -1, want_counts: bool = False):
        """Value of the criterion on the last train-mode forward without the backward (lseg_train_loss): the mean cross-entropy as a
        0-dim fp32 device tensor (no host sync) and, optionally, int64[2] = {correct, labeled} of the arg-max mask."""
        if self._groups is not None:
            check_ragged_target(target, len(self._groups), self.img_h, self.img_w)
        t = target.contiguous()
        assert t.dtype == torch.int64 and t.device == self.device
        self._loss_target = t                                     # the engine remembers the pointer for the following backward
        nll = torch.empty(2, dtype=torch.float64, device=self.device)
        cnt = torch.empty(2, dtype=torch.int64, device=self.device) if want_counts else None
        _lib.check(self.lib.lseg_train_loss(self._h, C.c_void_p(t.data_ptr()), ignore_index, C.c_void_p(nll.data_ptr()),
                                            C.c_void_p(cnt.data_ptr()) if cnt is not None else None,
                                            C.c_void_p(_stream_ptr(self.device))))
        loss = (nll[0] / nll[1]).float()
        return (loss, cnt) if want_counts else loss

    # ---- momentum buffers of the fused SGD (torch.optim.SGD state['momentum_buffer']; checkpoints, engine rebuilds) ----
    def _momentum_ptr(self, key: str):
        p, n = C.c_void_p(), C.c_size_t(0)
        _lib.check(self.lib.lseg_sgd_momentum(self._h, key.encode(), C.byref(p), C.byref(n)))
        return p.value, n.value

    def get_momentum(self, key: str) -> torch.Tensor:
        ptr, n = self._momentum_ptr(key)
        out = torch.empty(n, dtype=torch.float32, device=self.device)
        _HipMemcpy.copy(out.data_ptr(), ptr, 4 * n, _stream_ptr(self.device))
        return out.view(self.bound[key].shape)

    def set_momentum(self, key: str, value: torch.Tensor):
        ptr, n = self._momentum_ptr(key)
        v = value.detach().to(self.device, torch.float32).contiguous()
        if v.numel() != n:
            raise ValueError(f"momentum of '{key}' has {v.numel()} elements, expected {n}")
        _HipMemcpy.copy(ptr, v.data_ptr(), 4 * n, _stream_ptr(self.device))
        torch.cuda.current_stream(self.device).synchronize()       # v may be a temporary

    def mark_sgd_initialized(self, initialized: bool = True):
        _lib.check(self.lib.lseg_sgd_mark_initialized(self._h, int(initialized)))

    def sgd_step(self, lr_pretrained: float, lr_scratch: float, momentum: float = 0.9, weight_decay: float = 1e-4):
        """Fused SGD on the bound fp32 masters + re-pack of the engine's operand copies.  The masters (the caller's tensors) and the
        BatchNorm running statistics are written through raw pointers: tensor._version does NOT move -- other consumers of the
        same tensors (other engines of an LSegNet) must be told (LSeg.invalidate_engines)."""
        _lib.check(self.lib.lseg_sgd_step(self._h, lr_pretrained, lr_scratch, momentum, weight_decay,
                                          C.c_void_p(_stream_ptr(self.device))))

    # ---- fused Adam (torch.optim.Adam: state['exp_avg'], state['exp_avg_sq']; the step count stays with the caller) ----
    def _adam_ptr(self, key: str, which: int):
        p, n = C.c_void_p(), C.c_size_t(0)
        _lib.check(self.lib.lseg_adam_state(self._h, key.encode(), int(which), C.byref(p), C.byref(n)))
        return p.value, n.value

    def get_adam_state(self, key: str):
        """(exp_avg, exp_avg_sq) of a trainable parameter, copies in the parameter's shape."""
        out = []
        for which in (0, 1):
            ptr, n = self._adam_ptr(key, which)
            t = torch.empty(n, dtype=torch.float32, device=self.device)
            _HipMemcpy.copy(t.data_ptr(), ptr, 4 * n, _stream_ptr(self.device))
            out.append(t.view(self.bound[key].shape))
        return out[0], out[1]

    def set_adam_state(self, key: str, exp_avg: torch.Tensor, exp_avg_sq: torch.Tensor):
        for which, value in ((0, exp_avg), (1, exp_avg_sq)):
            ptr, n = self._adam_ptr(key, which)
            v = value.detach().to(self.device, torch.float32).contiguous()
            if v.numel() != n:
                raise ValueError(f"Adam state of '{key}' has {v.numel()} elements, expected {n}")
            _HipMemcpy.copy(ptr, v.data_ptr(), 4 * n, _stream_ptr(self.device))
            torch.cuda.current_stream(self.device).synchronize()   # v may be a temporary

    def adam_step(self, lr_pretrained: float, lr_scratch: float, step: int, betas=(0.9, 0.999), eps: float = 1e-8,
                  weight_decay: float = 0.0):
        """Fused torch.optim.Adam step (amsgrad / maximize off) on the bound fp32 masters + re-pack of the engine's operand copies;
        `step` is the count of this step, starting at 1.  Writes the masters through raw pointers, like sgd_step."""
        _lib.check(self.lib.lseg_adam_step(self._h, float(lr_pretrained), float(lr_scratch), float(betas[0]), float(betas[1]), float(eps),
                                           float(weight_decay), int(step), C.c_void_p(_stream_ptr(self.device))))

    def _guarded(self, fn):
        def call(*a):
            try:
                fn(*a)
            except BaseException as e:          # noqa: BLE001  (must not unwind through the C frames; re-raised by _raise_callback_error)
                if self._cb_error is None:
                    self._cb_error = e
        return call

    def set_bucket_callback(self, fn):
        """fn(bucket_index) is called on the host as soon as the bucket's last gradient kernel is enqueued."""
        g = self._guarded(fn) if fn is not None else None
        self._bucket_cb = _lib.BUCKET_CB(lambda user, b, stream: g(int(b))) if fn is not None else None
        _lib.check(self.lib.lseg_set_bucket_callback(self._h, C.cast(self._bucket_cb, C.c_void_p) if fn else None, None))

    def set_bn_sync(self, fn, world_size: int):
        """fn(dev_ptr, n_floats) must sum the n floats at dev_ptr over the ranks, ordered on the current stream."""
        g = self._guarded(fn) if fn is not None else None
        self._bn_cb = _lib.REDUCE_CB(lambda user, p, n, stream: g(int(p), int(n))) if fn is not None else None
        _lib.check(self.lib.lseg_set_bn_sync(self._h, C.cast(self._bn_cb, C.c_void_p) if fn else None, None, int(world_size)))

    def forward_stats(self, target: torch.Tensor, ignore_index: int = -1) -> dict:
        """pixAcc / IoU counts + CE sum of the last forward's output vs `target` int64 [B,H,W] (lseg_forward_stats): computed from the
        engine's low-resolution logits through the x2 bilinear on the fly -- pair it with forward(x, want_logits=False)."""
        t = target.detach().to(self.device, torch.int64).contiguous()
        K = self._group if self._group > 0 else self._K
        counts = torch.empty(2 + 3 * K, dtype=torch.int64, device=self.device)
        nll = torch.empty(2, dtype=torch.float64, device=self.device)
        _lib.check(self.lib.lseg_forward_stats(self._h, C.c_void_p(t.data_ptr()), int(ignore_index), C.c_void_p(counts.data_ptr()),
                                               C.c_void_p(nll.data_ptr()), C.c_void_p(_stream_ptr(self.device))))
        c, n = counts.cpu(), nll.cpu()
        inter, pred, lab = c[2:2 + K], c[2 + K:2 + 2 * K], c[2 + 2 * K:2 + 3 * K]
        return {"correct": int(c[0]), "labeled": int(c[1]), "area_inter": inter, "area_pred": pred, "area_lab": lab,
                "area_union": pred + lab - inter, "nll_sum": float(n[0]), "nll_count": int(n[1])}

    def label_stats(self, labels: torch.Tensor, target: torch.Tensor, ignore_index: int = -1, group_sizes=None, class_map=None, nclass=None,
                    out=None):
        """pixAcc / IoU counts of a label map this engine produced (forward_labels, shared or ragged) against `target` [B,H,W]
        (lseg_op_label_stats): DEVICE tensors (counts int64 [2 + 3n], flags int64 [2]), no host synchronisation.  The label set is the
        engine's current one: n = K for a shared set; with ragged per-image lists (set_tokens(group_sizes=...), or group_sizes given
        here) labels and targets index each image's own list and n = the number of list entries -- or nclass, when class_map gives every
        list entry its id in one vocabulary.  out = (counts, flags) of an earlier call: this batch is added to them."""
        from .metrics import label_stats
        if not torch.is_tensor(labels) or not torch.is_tensor(target):
            raise TypeError("label_stats: labels and target must be tensors")
        if labels.device != self.device or target.device != self.device:
            raise ValueError(f"label_stats: labels and target must live on {self.device} (no CPU path), got {labels.device} / {target.device}")
        if group_sizes is None and self._groups is not None:
            group_sizes = list(self._groups)
        if group_sizes is None and self._group > 0:
            group_sizes = [self._group] * labels.shape[0]
        return label_stats(labels, target, self._K if group_sizes is None else None, ignore_index, group_sizes, class_map, nclass, out)

    def episode_stats(self, target: torch.Tensor, ignore: Optional[torch.Tensor] = None, ignore_index: int = -100, class_id=None,
                      meter=None) -> dict:
        """Few-shot episode evaluation of the last forward's two label planes (lseg_episode_stats; inference or train-mode forward):
        Evaluator.classify_prediction(out.argmax(1), target, ignore) and the value of nn.CrossEntropyLoss() on `out`, per image, in one
        pass over the low-resolution logits -- pair it with forward(x, want_logits=False).  Returns DEVICE tensors in the reference's
        layout, no host synchronisation: area_inter / area_union int64 [2, B], nll_sum / nll_count float64 [B] (the criterion's value
        is nll_sum.sum() / nll_count.sum()), flags int64 [2] = {pixels with ignore set and target != 0, pixels whose target is outside
        {0, 1} and not ignore_index}, areas int64 [B, 6] = {inter0, inter1, pred0, pred1, gt0, gt1}.
        target [B,H,W] (any integer / float dtype holding 0 / 1, as the loaders give it); ignore [B,H,W] or None (non-zero = ignored).
        class_id + meter (lseg_hip.episode.EpisodeMeter): the same launch adds every image's inter / union into column class_id[b]
        of the meter (AverageMeter.update).  class_id is validated HERE, on the host: hand over the list the caller already has
        (net.forward reads class_info to pick the token pairs); a device tensor is read back, which synchronises."""
        t = target.detach().to(self.device, torch.int64).contiguous()
        if t.dim() != 3 or tuple(t.shape[1:]) != (self.img_h, self.img_w):
            raise ValueError(f"target must be [B, {self.img_h}, {self.img_w}], got {tuple(t.shape)}")
        B = t.shape[0]
        ig = None
        if ignore is not None:
            ig = ignore.detach().to(self.device)
            ig = (ig if ig.dtype == torch.uint8 else (ig != 0).to(torch.uint8)).contiguous()
            if ig.shape != t.shape:
                raise ValueError(f"ignore mask {tuple(ig.shape)} does not match the target {tuple(t.shape)}")
        cid = ib = ub = None
        nclass = 0
        if meter is not None:
            if class_id is None:
                raise ValueError("episode_stats: a meter needs class_id")
            ids = [int(c) for c in (class_id.tolist() if torch.is_tensor(class_id) else class_id)]
            nclass = int(meter.nclass)
            bad = [c for c in ids if not 0 <= c < nclass]
            if len(ids) != B or bad:
                raise _lib.LSegError(-1, f"episode_stats: class_id {ids} for a batch of {B}: every id must lie in [0, nclass={nclass})")
            if meter.intersection_buf.device != self.device:
                raise ValueError(f"the meter lives on {meter.intersection_buf.device}, the engine on {self.device}")
            cid = torch.tensor(ids, dtype=torch.int64).to(self.device, non_blocking=True)
            ib, ub = meter.intersection_buf, meter.union_buf
        areas = torch.empty((B, 6), dtype=torch.int64, device=self.device)
        nll = torch.empty((B, 2), dtype=torch.float64, device=self.device)
        flags = torch.empty(2, dtype=torch.int64, device=self.device)
        P = lambda x: C.c_void_p(x.data_ptr()) if x is not None else None          # noqa: E731
        _lib.check(self.lib.lseg_episode_stats(self._h, P(t), P(ig), int(ignore_index), P(cid), nclass, P(ib), P(ub), P(areas), P(nll),
                                               P(flags), C.c_void_p(_stream_ptr(self.device))))
        inter = areas[:, 0:2]
        out = {"area_inter": inter.t(), "area_union": (areas[:, 2:4] + areas[:, 4:6] - inter).t(), "nll_sum": nll[:, 0],
               "nll_count": nll[:, 1], "flags": flags, "areas": areas}
        if meter is not None:
            meter.note_scatter(flags, (nll[:, 0].sum() / nll[:, 1].sum()).float())
        return out

    # ---- taps / measurement ----------------------------------------------------------------------------
    def set_debug(self, enabled: bool):
        _lib.check(self.lib.lseg_set_debug(self._h, int(enabled)))

    def intermediate(self, name: str, shape: Sequence[int]) -> torch.Tensor:
        out = torch.empty(tuple(shape), dtype=torch.float32, device=self.device)
        n = C.c_size_t(0)
        _lib.check(self.lib.lseg_get_intermediate(self._h, name.encode(), C.c_void_p(out.data_ptr()),
                                                  out.numel(), C.byref(n), C.c_void_p(_stream_ptr(self.device))))
        if n.value != out.numel():
            raise ValueError(f"intermediate '{name}' has {n.value} elements, expected {out.numel()} {tuple(shape)}")
        return out

    def check_range(self) -> dict:
        """16-bit range check of the image tower (lseg_check_range): non-finite values, values within a factor 2 of the fp16 limit and
        the largest finite magnitude over every 16-bit activation buffer, as the forwards so far left them.  Synchronises."""
        import struct
        out = (C.c_uint64 * 4)()
        _lib.check(self.lib.lseg_check_range(self._h, out, C.c_void_p(_stream_ptr(self.device))))
        return {"nonfinite": int(out[0]), "near_fp16_limit": int(out[1]),
                "max_abs": struct.unpack("f", struct.pack("I", int(out[2]) & 0xffffffff))[0], "scanned": int(out[3])}

    def overflow_seen(self, reset: bool = False) -> bool:
        """True once a COMPLETED inference forward left inf / NaN in the head feature map (lseg_overflow_seen: no synchronisation; an overflow on
        one call is reported at the latest by the next one).  Sticky until reset."""
        r = self.lib.lseg_overflow_seen(self._h, int(reset))
        if r < 0:
            _lib.check(r)
        return bool(r)

    PROFILE_FAMILIES = ("forward", "mlp_fc1", "mlp_fc2", "attn_proj", "attn_qkv", "attention", "layernorm", "correlation")

    def set_profiling(self, enabled):
        """True = HIP-event timing of the whole forward + the MLP fc1 GEMM; a list of family names (PROFILE_FAMILIES) = exactly those;
        False = off.  The events are created here, outside any timed region (lseg_set_profiling)."""
        if isinstance(enabled, (list, tuple, set)):
            mask = 1 << 30               # an unused family bit: keeps a one-family mask apart from the ABI's "1 = forward + mlp_fc1"
            for f in enabled:
                mask |= 1 << self.PROFILE_FAMILIES.index(f)
        else:
            mask = int(bool(enabled))
        _lib.check(self.lib.lseg_set_profiling(self._h, mask))

    def profile(self, family: str):
        ms, n, fl = C.c_double(0), C.c_int64(0), C.c_double(0)
        _lib.check(self.lib.lseg_get_profile(self._h, family.encode(), C.byref(ms), C.byref(n), C.byref(fl)))
        return {"total_ms": ms.value, "launches": n.value, "flops_per_launch": fl.value}
