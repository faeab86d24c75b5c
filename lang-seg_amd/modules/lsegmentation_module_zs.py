"""LSegmentationModuleZS -- mirror of the reference's modules/lsegmentation_module_zs.py:38-343, network / criterion / optimizer side.

What is mirrored: the learning-rate rule (`base_lr / 16 * batch_size`, :43), `fixed_encoder` for use_pretrained == 'clip_fixed' (:50),
`forward(x, class_info)` (:82-83), the 2-class `criterion` (:338-343), `training_step` for the reference's three batch layouts
(:86-155: finetune 5-shot, finetune 1-shot, support + query) and `configure_optimizers` (:218-293: SGD momentum 0.9 + weight decay under
the poly LambdaLR, the same parameter groups including the empty `auxlayer` one and the clip_fixed groups).

The optimizer is EngineSGD, or EngineAdam with midasproto (modules/lsegmentation_module.py): after an engine backward its step is the
engine's fused lseg_sgd_step / lseg_adam_step when the live groups are exactly {pretrained.*, scratch.*} -- the non-frozen layout, the
empty `auxlayer` group counting as absent.  The clip_fixed layout (pretrained.model at lr 0, act_postprocess1..4 at base_lr, scratch at
10x) is not that shape and by default takes torch's own step on the engine's gradients: lr 0 leaves pretrained.model.* bit-identical,
and as in the reference the ViT's gradients are still computed.

skip_frozen_backward=True (opt-in, only with use_pretrained == 'clip_fixed'): the network's training engines freeze the encoder
(LSegNetZS(freeze_encoder=True) -> lseg_set_frozen_encoder) -- the backward stops at the four readouts, the same six groups come back
from configure_optimizers, and the optimizer's fused step accepts them.  DIFFERENCE from the default path: the .grad of every
pretrained.model.* parameter stays None (the default path fills it with gradients that the lr-0 group then ignores).

Not mirrored (host-side data plumbing, SURVEY.md §8 out of scope): the few-shot FSSDataset loaders, Logger, AverageMeter, Evaluator and
the few-shot IoU bookkeeping of training_step / validation_step.
"""
import torch
import torch.nn as nn

from .lsegmentation_module import _Base, EngineAdam, EngineSGD


class LSegmentationModuleZS(_Base):
    def __init__(self, data_path, dataset, batch_size, base_lr, max_epochs, **kwargs):
        super().__init__()
        self.data_path, self.dataset = data_path, dataset
        self.batch_size = batch_size
        self.base_lr = base_lr / 16 * batch_size              # :43
        self.lr = self.base_lr
        self.epochs = max_epochs
        self.other_kwargs = kwargs
        self.enabled = False                                  # AMP off (:47): the reference's GradScaler(enabled=False).scale is the identity
        self.fixed_encoder = kwargs.get("use_pretrained") in ["clip_fixed"]     # :50
        # opt-in: do not compute the gradients the lr-0 group of clip_fixed discards (pretrained.model.*.grad stays None in this mode)
        self.skip_frozen_backward = bool(kwargs.get("skip_frozen_backward", False)) and self.fixed_encoder
        self.cross_entropy_loss = nn.CrossEntropyLoss()       # :53 (ignore_index = -100, mean)
        self.nshot = kwargs.get("nshot", 1)
        self.finetune_mode = kwargs.get("finetune_mode", False)
        self.num_classes = 2
        self.labels = ["others", ""]

    def forward(self, x, class_info):                         # :82-83
        return self.net(x, class_info)

    def criterion(self, logit_mask, gt_mask):                 # :338-343
        bsz = logit_mask.size(0)
        logit_mask = logit_mask.view(bsz, 2, -1)
        gt_mask = gt_mask.view(bsz, -1).long()
        return self.cross_entropy_loss(logit_mask, gt_mask)

    def batch_inputs(self, batch):
        """(img, target, class_info) of a few-shot batch, the reference's three layouts (:87-135)."""
        if self.finetune_mode:
            if self.nshot == 5:                               # :88-96 (class_id repeated shot-major, as the reference does)
                bshape = batch["support_imgs"].shape
                img = batch["support_imgs"].view(-1, bshape[2], bshape[3], bshape[4])
                target = batch["support_masks"].view(-1, bshape[3], bshape[4])
                class_info = batch["class_id"]
                for _ in range(1, 5):
                    class_info = torch.cat([class_info, batch["class_id"]])
            else:                                             # :108-112
                img = batch["support_imgs"].squeeze(1)
                target = batch["support_masks"].squeeze(1)
                class_info = batch["class_id"]
        else:                                                 # :126-128: support + query
            img = torch.cat([batch["support_imgs"].squeeze(1), batch["query_img"]], dim=0)
            target = torch.cat([batch["support_masks"].squeeze(1), batch["query_mask"]], dim=0)
            class_info = torch.cat([batch["class_id"], batch["class_id"]], dim=0)
        return img, target, class_info

    def _fused_ignore_index(self):
        """ignore_index when the criterion is the plain mean cross-entropy the engine's fused loss implements, else None."""
        c = self.cross_entropy_loss
        if not isinstance(c, nn.CrossEntropyLoss) or c.weight is not None or c.reduction != "mean" or getattr(c, "label_smoothing", 0.0) != 0.0:
            return None
        if type(self).criterion is not LSegmentationModuleZS.criterion:
            return None
        return int(c.ignore_index)

    def training_step(self, batch, batch_nb):                 # :86-155 (loss part)
        img, target, class_info = self.batch_inputs(batch)
        ignore = self._fused_ignore_index()
        if ignore is not None and hasattr(self.net, "forward_loss") and not self.other_kwargs.get("materialize_logits", False):
            # `out = self(img, class_info); loss = self.criterion(out, target)` as ONE autograd node on the engine (no [B, 2, H, W] logits)
            t = target.reshape(img.shape[0], img.shape[2], img.shape[3]).long()
            loss = self.net.forward_loss(img, class_info, t, ignore_index=ignore)
        else:
            out = self(img, class_info)
            loss = self.criterion(out, target)
        self.log("train_loss", loss)
        return loss

    def configure_optimizers(self):                           # :218-293
        net = self.net
        if self.fixed_encoder:
            params_list = [{"params": net.pretrained.model.parameters(), "lr": 0}]
            for i in (1, 2, 3, 4):
                params_list.append({"params": getattr(net.pretrained, f"act_postprocess{i}").parameters(), "lr": self.base_lr})
        else:
            params_list = [{"params": net.pretrained.parameters(), "lr": self.base_lr}]
        if hasattr(net, "scratch"):
            params_list.append({"params": net.scratch.parameters(), "lr": self.base_lr * 10})
        if hasattr(net, "auxlayer"):
            params_list.append({"params": net.auxlayer.parameters(), "lr": self.base_lr * 10})
        if self.other_kwargs.get("midasproto", False):        # :270-281
            opt = EngineAdam(params_list, net=net, lr=self.base_lr, betas=(0.9, 0.999), weight_decay=self.other_kwargs.get("weight_decay", 1e-4))
        else:
            opt = EngineSGD(params_list, net=net, lr=self.base_lr, momentum=0.9, weight_decay=self.other_kwargs.get("weight_decay", 1e-4))
        sch = torch.optim.lr_scheduler.LambdaLR(opt, lambda x: pow(1.0 - x / self.epochs, 0.9))
        return [opt], [sch]
