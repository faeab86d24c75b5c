"""LSegNetZS -- drop-in for the reference's zero-shot network, modules/models/lseg_net_zs.py:106-214, 217-240.

Same constructor surface (`LSegNetZS(label_list, path=None, scale_factor=0.5, aux=False, use_relabeled=False,
use_pretrained=True, **kwargs)`), same module tree / state-dict keys as LSegNet, same
`forward(x, class_info) -> float32 [B, 2, H, W]`: image b is scored against ITS OWN label pair
['others', label_list[class_info[b]]] (`self.texts`, lseg_net_zs.py:170-176, 178).  The arithmetic runs in the HIP engine
with per-image label grouping (include/lseg_hip.h: lseg_set_text_grouping); there is no PyTorch fallback.

Training (LSegmentationModuleZS.training_step, modules/lsegmentation_module_zs.py): under net.train() with grad enabled the
forward is the engine's train-mode step with the same grouping -- one autograd node whose backward is lseg_backward(d logits), exactly
as LSegNet's -- and `forward_loss(x, class_info, target)` is criterion(forward(x, class_info), target) as ONE node (fused
cross-entropy over the 2 label planes, no [B, 2, H, W] logits).

LSegRNNetZS (lseg_net_zs.py:243-363) is the same network on the clip_resnet101 backbone: torchvision's ResNet-101 as the image
tower (lseg_config.flags bit 5, csrc/resnet.hip), the neck, head and CLIP ViT-B/32 text tower as above.  By default it is inference
only and its train-mode forward raises; LSegRNNetZS(..., train_decoder=True) trains the decoder above the tower (scratch.*) with the
tower in train() mode: batch-statistics BatchNorm, running buffers updated, no gradient for pretrained.* (their .grad stays None).
"""
import numpy as np
from collections import OrderedDict

import torch
import torch.nn as nn

from lseg_hip.config import get_config
from lseg_hip.engine import image_dims
from lseg_hip.tokenizer import tokenize
from .lseg_blocks import Interpolate, _make_encoder
from .lseg_net import BaseModel, default_image_dtype, LSeg as _LSegShared, _make_fusion_block, _new_shared, _EngineTrainFn, _EngineLossFn


class LSeg(_LSegShared):
    def __init__(self, head, features=256, backbone="clip_vitl16_384", readout="project", channels_last=False,
                 use_bn=False, **kwargs):
        BaseModel.__init__(self)
        self.channels_last = channels_last
        if readout != "project":
            raise NotImplementedError("the HIP engine implements readout='project' (the only mode LSegNetZS uses)")
        if kwargs.get("arch_option", 0) not in (0, None):
            # the reference stores arch_option but LSeg.forward of the ZS net never runs head blocks (:177-214)
            pass
        self.arch_option = kwargs.get("arch_option", 0)
        self.block_depth = 0
        self.cfg = get_config(backbone, features=features, arch_option=0, block_depth=0,
                              activation=kwargs.get("activation", "lrelu") or "lrelu")
        self.clip_pretrained, self.pretrained, self.scratch = _make_encoder(self.cfg)
        for r in (1, 2, 3, 4):
            setattr(self.scratch, f"refinenet{r}", _make_fusion_block(features, use_bn))
        self.auxlayer = nn.Sequential(Interpolate(scale_factor=2, mode="bilinear", align_corners=True))   # :150-152
        self.logit_scale = nn.Parameter(torch.ones([]) * np.log(1 / 0.07)).exp()                           # :155
        self.out_c = self.cfg.out_c
        self.scratch.head1 = nn.Conv2d(features, self.out_c, kernel_size=1)
        self.scratch.output_conv = head
        # one token pair per class: ['others', <class name>]  (:169-176)
        self.texts = [tokenize(["others", name], self.cfg.text.ctx, self.cfg.text.vocab) for name in self.label_list]
        self._engines = OrderedDict()
        self.max_engines = kwargs.get("max_engines", 4)
        self._shared = _new_shared(kwargs.get("image_dtype", default_image_dtype()))
        self.overflow_fallback = kwargs.get("overflow_fallback", True)      # fp16 range check + loud bf16 fallback, as LSegNet (lseg_net.py)
        self.cache_text = kwargs.get("cache_text", False)
        self.autograd_grads = False
        self.sync_batchnorm = False
        self._native_epoch = 0
        self._last_train_counts = None
        self.freeze_encoder = bool(kwargs.get("freeze_encoder", False))      # as LSegNet: training engines skip the encoder backward

    def forward(self, x, class_info):
        ids = [int(c) for c in (class_info.tolist() if torch.is_tensor(class_info) else class_info)]
        if not x.is_cuda:
            raise RuntimeError("LSegNetZS.forward needs a CUDA/HIP tensor (no CPU path, no PyTorch fallback)")
        B, H, W = image_dims(x)
        if len(ids) != B:
            raise ValueError(f"class_info has {len(ids)} entries for a batch of {B}")
        if self.training and torch.is_grad_enabled():                         # training_step (lsegmentation_module_zs.py:86-155)
            eng, keys, params = self._train_inputs(x, ids)
            return _EngineTrainFn.apply(self._input(eng, x), self, eng, keys, *params)
        text = torch.cat([self.texts[c] for c in ids], dim=0)                 # [2B, ctx]; :178
        eng = self._engine(B, H, W, text.shape[0], x.device)
        if eng.training:
            eng.set_train(False)
        self._set_group_tokens(eng, text, ids)
        out = eng.forward(self._input(eng, x))                                          # [B, 2, H, W]
        if self._range_guard(eng, x.device):
            return self.forward(x, class_info)                                # fp16 overflowed: again on bf16 operands (loud)
        return out

    def evaluate_episode(self, x, class_info, target, ignore=None, meter=None, want_logits=False):
        """One few-shot evaluation step on the device -- `out = self(x, class_info)`, Evaluator.classify_prediction(out.argmax(1),
        target, ignore), criterion(out, target) and, with a meter (lseg_hip.episode.EpisodeMeter), AverageMeter.update -- as
        test_lseg_zs.py:289-312 / LSegmentationModuleZS.validation_step (:157-192) do it: an inference forward that keeps only the
        low-resolution logits, then lseg_episode_stats.  Returns (area_inter int64 [2, B], area_union int64 [2, B], loss) -- loss a
        0-dim fp32 device tensor = sum(nll_sum) / sum(nll_count), nn.CrossEntropyLoss()'s mean -- and, with want_logits, the
        [B, 2, H, W] logits as a fourth item.  No host synchronisation beyond the range guard's (as in forward)."""
        ids = [int(c) for c in (class_info.tolist() if torch.is_tensor(class_info) else class_info)]
        if not x.is_cuda:
            raise RuntimeError("LSegNetZS.evaluate_episode needs a CUDA/HIP tensor (no CPU path, no PyTorch fallback)")
        B, H, W = image_dims(x)
        if len(ids) != B:
            raise ValueError(f"class_info has {len(ids)} entries for a batch of {B}")
        text = torch.cat([self.texts[c] for c in ids], dim=0)
        eng = self._engine(B, H, W, text.shape[0], x.device)
        if eng.training:
            eng.set_train(False)
        self._set_group_tokens(eng, text, ids)
        out = eng.forward(self._input(eng, x), want_logits=bool(want_logits))            # None without logits: only the low planes stay
        if self._range_guard(eng, x.device):
            return self.evaluate_episode(x, class_info, target, ignore, meter, want_logits)    # fp16 overflowed: again on bf16 operands
        r = eng.episode_stats(target.reshape(B, H, W), None if ignore is None else ignore.reshape(B, H, W),
                              ignore_index=-100, class_id=ids, meter=meter)
        loss = (r["nll_sum"].sum() / r["nll_count"].sum()).float()
        res = (r["area_inter"], r["area_union"], loss)
        return res + (out,) if want_logits else res

    def _set_group_tokens(self, eng, text, ids):
        tkey = ("zs", tuple(ids))
        if eng._tok != tkey:
            eng.set_tokens(text, labels_per_image=2)
            eng._tok = tkey
        eng.set_text_cache(bool(self.cache_text))

    def _train_inputs(self, x, class_info):
        """The train-mode engine of this batch shape with the per-image token pairs set (LSeg._train_inputs with class_info in place
        of a label set): the text tower still runs per step on its side stream -- the pairs change with class_info."""
        if not x.is_cuda:
            raise RuntimeError("LSegNetZS needs CUDA/HIP tensors (no CPU path)")
        ids = [int(c) for c in (class_info.tolist() if torch.is_tensor(class_info) else class_info)]
        B, H, W = image_dims(x)
        if len(ids) != B:
            raise ValueError(f"class_info has {len(ids)} entries for a batch of {B}")
        text = torch.cat([self.texts[c] for c in ids], dim=0)
        eng = self._train_engine(B, H, W, text.shape[0], x.device)
        self._set_group_tokens(eng, text, ids)
        if eng._nbt:
            torch._foreach_add_(eng._nbt, 1)             # nn.BatchNorm2d.num_batches_tracked
        self.invalidate_engines(except_=eng)             # train-mode BatchNorm moves the running statistics through raw pointers
        return eng, tuple(k for k, _ in eng._named), [p for _, p in eng._named]

    def forward_loss(self, x, class_info, target, ignore_index=-100):
        """`criterion(self(x, class_info), target)` of LSegmentationModuleZS (nn.CrossEntropyLoss() over [B, 2, H*W]: mean over the
        pixels != ignore_index, torch's default -100) as ONE autograd node on the engine: no [B, 2, H, W] logits; `loss.backward()`
        runs lseg_backward_scaled.  Leaves {correct, labeled} of the batch in `self._last_train_counts` (int64[2], device)."""
        if not (self.training and torch.is_grad_enabled()):
            raise RuntimeError("forward_loss is the training-step path: call it under net.train() with grad enabled")
        eng, keys, params = self._train_inputs(x, class_info)
        self._last_train_engine = eng                    # holds this step's train-mode logits: LSegmentationModuleZS's train_average_meter
        return _EngineLossFn.apply(self._input(eng, x), target, self, eng, keys, int(ignore_index), *params)


class LSegNetZS(LSeg):
    """Network for zero-shot semantic segmentation (lseg_net_zs.py:217-240)."""

    def __init__(self, label_list, path=None, scale_factor=0.5, aux=False, use_relabeled=False, use_pretrained=True,
                 **kwargs):
        features = kwargs["features"] if "features" in kwargs else 256
        kwargs["use_bn"] = True
        self.scale_factor = scale_factor
        self.aux = aux
        self.use_relabeled = use_relabeled
        self.label_list = label_list
        self.use_pretrained = use_pretrained
        head = nn.Sequential(Interpolate(scale_factor=2, mode="bilinear", align_corners=True))
        super().__init__(head, **kwargs)
        if path is not None:
            self.load(path)


class LSegRNNetZS(LSeg):
    """Zero-shot network on the CLIP-ResNet-101 backbone (lseg_net_zs.py:243-363): the reference's LSegRN module tree
    (clip_pretrained = CLIP ViT-B/32, pretrained.layer1..4 = torchvision ResNet-101, scratch with BN refinenets, head1, output_conv)
    and `forward(x, class_info) -> float32 [B, 2, H, W]` through the HIP engine.  Inference only unless built with train_decoder=True:
    then `net.train()` forwards return logits with LSegNetZS's autograd node and `forward_loss` is offered -- the reference's few-shot
    training step with the `pretrained` group inert: scratch.layerN_rn, the refinenets and head1 get gradients, the tower's BatchNorms
    normalise with batch statistics and write the running buffers of this module's own nn.BatchNorm2d tensors."""

    def __init__(self, label_list=None, path=None, scale_factor=0.5, aux=False, use_relabeled=False, use_pretrained=True, **kwargs):
        self.train_decoder = bool(kwargs.pop("train_decoder", False))
        if label_list is None:
            raise NotImplementedError("LSegRNNetZS needs a label_list (one ['others', label] token pair per class)")
        features = kwargs["features"] if "features" in kwargs else 256
        kwargs["use_bn"] = True
        kwargs["backbone"] = kwargs.get("backbone", "clip_resnet101")
        if kwargs["backbone"] != "clip_resnet101":
            raise NotImplementedError(f"LSegRNNetZS implements backbone='clip_resnet101' (got {kwargs['backbone']!r})")
        self.scale_factor = scale_factor
        self.aux = aux
        self.use_relabeled = use_relabeled
        self.label_list = label_list
        self.use_pretrained = use_pretrained
        head = nn.Sequential(Interpolate(scale_factor=2, mode="bilinear", align_corners=True))
        super().__init__(head, **kwargs)
        if path is not None:
            self.load(path)

    def forward(self, x, class_info):
        if self.training and torch.is_grad_enabled() and not self.train_decoder:
            raise NotImplementedError("LSegRNNetZS is inference only (the ResNet-101 tower has no train-mode BatchNorm / backward): "
                                      "call net.eval() or run under torch.no_grad()")
        return super().forward(x, class_info)

    def forward_loss(self, x, class_info, target, ignore_index=-100):
        if not self.train_decoder:
            raise NotImplementedError("LSegRNNetZS is inference only")
        return super().forward_loss(x, class_info, target, ignore_index)
