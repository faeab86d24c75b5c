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

The few-shot episode evaluation (:100-143, :157-216): `validation_step` / `validation_epoch_end` and, when the module carries a
`train_average_meter`, the IoU bookkeeping of `training_step` run on the device -- LSeg.evaluate_episode / HipEngine.episode_stats
(csrc/episode.hip) in place of Evaluator.classify_prediction, lseg_hip.episode.EpisodeMeter in place of AverageMeter.  The meters are
attached by the caller (`module.val_average_meter = EpisodeMeter(benchmark, dataset.class_ids, device)`), who owns the dataset.
Three differences from the reference: the meter keeps exact int64 areas (the reference's float32 buffers stop being exact above 2^24
pixels per class); the reference's `assert` on ignored-and-labelled pixels is a ValueError raised by compute_iou() in
validation_epoch_end (no per-batch synchronisation); validation_epoch_end carries neither the reference's `exit()` after epoch 3
(:204-216) nor its tensorboard writer.

Not mirrored (host-side data plumbing, SURVEY.md §8 out of scope): the few-shot FSSDataset loaders, Logger (write_process /
write_result) and visualisation.
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
        fused = ignore is not None and hasattr(self.net, "forward_loss") and not self.other_kwargs.get("materialize_logits", False)
        if fused:
            # `out = self(img, class_info); loss = self.criterion(out, target)` as ONE autograd node on the engine (no [B, 2, H, W] logits)
            t = target.reshape(img.shape[0], img.shape[2], img.shape[3]).long()
            loss = self.net.forward_loss(img, class_info, t, ignore_index=ignore)
        else:
            out = self(img, class_info)
            loss = self.criterion(out, target)
        self.log("train_loss", loss)
        meter = getattr(self, "train_average_meter", None)
        if meter is not None:                                 # :100-137: Evaluator.classify_prediction + AverageMeter.update, on the device
            self._train_meter_update(meter, batch, img, target, class_info, loss, fused)
        return loss

    def _train_meter_update(self, meter, batch, img, target, class_info, loss, fused):
        """The IoU bookkeeping of training_step on the train-mode forward's own logits (lseg_episode_stats after forward_loss: the
        engine still holds them).  Needs the fused step; with materialize_logits or a custom criterion it raises."""
        B, H, W = img.shape[0], img.shape[2], img.shape[3]
        ignore = self.train_ignore_mask(batch)
        ids = [int(c) for c in class_info.tolist()]
        eng = getattr(self.net, "_last_train_engine", None) if fused else None
        if eng is None:
            raise RuntimeError("train_average_meter needs the fused training step (net.forward_loss): detach the meter or drop materialize_logits")
        eng.episode_stats(target.reshape(B, H, W), None if ignore is None else ignore.reshape(B, H, W), ignore_index=self._fused_ignore_index(),
                          class_id=ids, meter=meter)
        meter.loss_buf[-1] = loss.detach().clone()            # the reference stores the step's own loss (:137)

    def train_ignore_mask(self, batch):
        """The ignore mask of a training batch in batch_inputs' layout, or None: only for benchmark 'pascal' and when the batch
        carries one (:101-102, :116-117, :132-133)."""
        if self.dataset != "pascal":                          # self.args.benchmark = dataset (:60)
            return None
        if self.finetune_mode:
            ig = batch.get("support_ignore_idxs")
            if ig is None:
                return None
            return ig.reshape(-1, ig.shape[-2], ig.shape[-1]) if self.nshot == 5 else ig.squeeze(1)
        if batch.get("query_ignore_idx") is None:
            return None
        return torch.cat([batch["support_ignore_idxs"].squeeze(1), batch["query_ignore_idx"]], dim=0)

    def validation_batch_inputs(self, batch):
        """(img, target, class_info, ignore) of a validation batch, the reference's two layouts (:158-184): the 5-shot finetune
        `view(-1, ...)` with class_id repeated shot-major, and the query layout.  ignore is None unless benchmark == 'pascal' and the
        batch carries `query_ignore_idx` (:168, :180)."""
        ig = batch.get("query_ignore_idx") if self.dataset == "pascal" else None      # self.args.benchmark = dataset (:60)
        if self.finetune_mode and self.nshot == 5:            # :158-164
            bshape = batch["query_img"].shape
            img = batch["query_img"].view(-1, bshape[2], bshape[3], bshape[4])
            target = batch["query_mask"].view(-1, bshape[3], bshape[4])
            class_info = batch["class_id"]
            for _ in range(1, 5):
                class_info = torch.cat([class_info, batch["class_id"]])
            if ig is not None:
                ig = ig.view(-1, bshape[3], bshape[4])
        else:                                                 # :174-176
            img = batch["query_img"].squeeze(1)
            target = batch["query_mask"].squeeze(1)
            class_info = batch["class_id"]
            if ig is not None:
                ig = ig.squeeze(1)
        return img, target, class_info, ig

    def validation_step(self, batch, batch_nb):               # :157-192
        """out = self(img, class_info); val_loss = criterion(out, target); Evaluator.classify_prediction; val_average_meter.update --
        one inference forward and one statistics launch on the device (LSeg.evaluate_episode).  Without the reference's
        write_process logging (Logger is not mirrored)."""
        meter = getattr(self, "val_average_meter", None)
        if meter is None:
            raise RuntimeError("validation_step needs `module.val_average_meter = lseg_hip.episode.EpisodeMeter(benchmark, dataset.class_ids, device)`")
        img, target, class_info, ignore = self.validation_batch_inputs(batch)
        _, _, val_loss = self.net.evaluate_episode(img, class_info, target, ignore=ignore, meter=meter)
        return val_loss

    def validation_epoch_end(self, outs):                     # :195-202 (no exit() after epoch 3, no tensorboard writer: :204-216)
        meter = self.val_average_meter
        val_loss = torch.stack(meter.loss_buf).mean() if meter.loss_buf else torch.zeros(())
        val_miou, val_fb_iou = meter.compute_iou()            # raises ValueError on ignored-and-labelled pixels / targets outside {0, 1}
        self.log("fewshot_val_loss", val_loss)
        self.log("fewshot_val_miou", val_miou)
        self.log("fewshot_val_fb_iou", val_fb_iou)

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
