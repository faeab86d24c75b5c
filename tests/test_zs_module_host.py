"""LSegmentationModuleZS on the host (no GPU): the optimizer groups and learning rates of the reference's configure_optimizers
(modules/lsegmentation_module_zs.py:218-293), the base-lr rule (:43), the criterion (:338-343), the three batch layouts of
training_step (:86-135), and EngineSGD's rule that an empty group counts as absent."""
import warnings

import pytest
import torch
import torch.nn.functional as F


def _module(use_pretrained="False", batch_size=4, base_lr=0.004, **kw):
    warnings.simplefilter("ignore")
    from modules.lseg_module_zs import LSegModuleZS
    return LSegModuleZS("nowhere", "fss", batch_size, base_lr, 20, backbone="tiny16", num_features=64, arch_option=0, block_depth=0,
                        activation="lrelu", use_pretrained=use_pretrained, aux=False, weight_decay=1e-4, **kw)


def _ids(params):
    return {id(p) for p in params}


def test_configure_optimizers_matches_the_reference_groups():
    from modules.lsegmentation_module import EngineSGD
    from modules.lsegmentation_module_zs import LSegmentationModuleZS
    m = _module(batch_size=4, base_lr=0.004)
    assert isinstance(m, LSegmentationModuleZS)
    assert m.base_lr == pytest.approx(0.004 / 16 * 4) and not m.fixed_encoder
    (opt,), (sch,) = m.configure_optimizers()
    assert isinstance(opt, EngineSGD) and isinstance(sch, torch.optim.lr_scheduler.LambdaLR)
    g = opt.param_groups
    # pretrained at base_lr, scratch at 10x, the auxlayer group (an Interpolate: no parameters) at 10x
    assert len(g) == 3
    assert [x["lr"] for x in g] == pytest.approx([m.base_lr, 10 * m.base_lr, 10 * m.base_lr])
    assert _ids(g[0]["params"]) == _ids(m.net.pretrained.parameters())
    assert _ids(g[1]["params"]) == _ids(m.net.scratch.parameters())
    assert len(g[2]["params"]) == 0
    assert all(x["momentum"] == 0.9 and x["weight_decay"] == 1e-4 for x in g)
    # the empty group counts as absent: the two live groups are the fused step's {pretrained.*, scratch.*}
    assert len(opt._live_groups()) == 2 and opt._fusable()
    # poly schedule (:281-283)
    opt.step()
    sch.step()
    assert g[0]["lr"] == pytest.approx(m.base_lr * (1 - 1 / 20) ** 0.9)


def test_configure_optimizers_clip_fixed_groups():
    m = _module(use_pretrained="clip_fixed", batch_size=8, base_lr=0.01)
    assert m.fixed_encoder and m.base_lr == pytest.approx(0.01 / 16 * 8)
    (opt,), _ = m.configure_optimizers()
    g = opt.param_groups
    # pretrained.model at lr 0, act_postprocess1..4 at base_lr, scratch at 10x, auxlayer (empty) at 10x
    assert len(g) == 7
    assert [x["lr"] for x in g] == pytest.approx([0.0] + [m.base_lr] * 4 + [10 * m.base_lr] * 2)
    assert _ids(g[0]["params"]) == _ids(m.net.pretrained.model.parameters())
    for i in range(4):
        assert _ids(g[1 + i]["params"]) == _ids(getattr(m.net.pretrained, f"act_postprocess{i + 1}").parameters())
    assert _ids(g[5]["params"]) == _ids(m.net.scratch.parameters()) and len(g[6]["params"]) == 0
    # not the fused step's shape: torch's SGD takes these steps (lr 0 leaves the frozen encoder where it is)
    assert not opt._fusable()


def test_engine_sgd_ignores_only_empty_groups():
    from modules.lsegmentation_module import EngineSGD
    a, b, c = (torch.nn.Parameter(torch.zeros(3)) for _ in range(3))
    assert EngineSGD([{"params": [a]}, {"params": [b]}], lr=0.1, momentum=0.9)._fusable()
    assert EngineSGD([{"params": [a]}, {"params": [b]}, {"params": []}], lr=0.1, momentum=0.9)._fusable()
    assert not EngineSGD([{"params": [a]}, {"params": [b]}, {"params": [c]}], lr=0.1, momentum=0.9)._fusable()


def test_criterion_is_two_class_cross_entropy():
    m = _module()
    g = torch.Generator().manual_seed(0)
    logits = torch.randn(3, 2, 8, 6, generator=g)
    target = torch.randint(0, 2, (3, 8, 6), generator=g).float()          # few-shot masks arrive as floats
    assert torch.allclose(m.criterion(logits, target), F.cross_entropy(logits, target.long()))
    assert m._fused_ignore_index() == -100


@pytest.mark.parametrize("layout", ["finetune_5shot", "finetune_1shot", "support_query"])
def test_training_step_batch_layouts(layout):
    kw = {"finetune_5shot": dict(finetune_mode=True, nshot=5), "finetune_1shot": dict(finetune_mode=True, nshot=1),
          "support_query": dict(finetune_mode=False, nshot=1)}[layout]
    m = _module(**kw)
    B, H, W = 2, 16, 16
    g = torch.Generator().manual_seed(1)
    cls = torch.tensor([3, 7])
    if layout == "finetune_5shot":
        batch = {"support_imgs": torch.randn(B, 5, 3, H, W, generator=g), "support_masks": torch.randint(0, 2, (B, 5, H, W), generator=g),
                 "class_id": cls}
    else:
        batch = {"support_imgs": torch.randn(B, 1, 3, H, W, generator=g), "support_masks": torch.randint(0, 2, (B, 1, H, W), generator=g),
                 "query_img": torch.randn(B, 3, H, W, generator=g), "query_mask": torch.randint(0, 2, (B, H, W), generator=g), "class_id": cls}
    img, target, class_info = m.batch_inputs(batch)
    if layout == "finetune_5shot":
        assert img.shape == (10, 3, H, W) and target.shape == (10, H, W)
        assert class_info.tolist() == [3, 7] * 5                           # repeated shot-major, as the reference concatenates it
        assert torch.equal(img[1], batch["support_imgs"][0, 1])
    elif layout == "finetune_1shot":
        assert img.shape == (2, 3, H, W) and class_info.tolist() == [3, 7]
    else:
        assert img.shape == (4, 3, H, W) and class_info.tolist() == [3, 7, 3, 7]
        assert torch.equal(img[2], batch["query_img"][0]) and torch.equal(target[3], batch["query_mask"][1])
