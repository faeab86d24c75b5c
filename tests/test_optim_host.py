"""The optimizers of the training modules on the host (no GPU): `--midasproto` returns EngineAdam -- a torch.optim.Adam with the
reference's groups, learning rates, betas and weight decay (modules/lsegmentation_module.py:152-163,
modules/lsegmentation_module_zs.py:270-281) --, EngineAdam without an engine IS torch's Adam, the clip_fixed group layout
(lsegmentation_module_zs.py:220-235) is a fused-step layout only for a frozen-encoder engine, and the new C entry points are declared,
exported and bound with matching arity."""
import copy
import os
import re
import types
import warnings

import pytest
import torch

NEW_SYMBOLS = {"lseg_adam_step": 9, "lseg_adam_state": 5, "lseg_set_frozen_encoder": 2}


def _zs_module(use_pretrained="False", **kw):
    warnings.simplefilter("ignore")
    from modules.lseg_module_zs import LSegModuleZS
    return LSegModuleZS("nowhere", "fss", 4, 0.004, 20, backbone="tiny16", num_features=64, arch_option=0, block_depth=0,
                        activation="lrelu", use_pretrained=use_pretrained, aux=False, weight_decay=1e-4, **kw)


def _seg_module(**kw):
    warnings.simplefilter("ignore")
    from modules.lsegmentation_module import LSegmentationModule
    from modules.models.lseg_net import LSegNet
    m = LSegmentationModule("nowhere", "ade20k", 4, 0.004, 20, weight_decay=1e-4, ignore_index=-1, **kw)
    m.net = LSegNet(labels=["wall", "sky", "tree"], backbone="tiny16", features=64, arch_option=0, block_depth=0, activation="lrelu")
    return m


def _ids(params):
    return {id(p) for p in params}


def _stub_engine(net, frozen):
    """What _groups_match reads of a training engine: the keys with a gradient buffer and the frozen-encoder flag."""
    never = lambda k: k.startswith(("pretrained.model.norm.", "pretrained.model.head.")) or ".refinenet4.resConfUnit1." in k
    keys = [k for k, _ in net.named_parameters() if k.startswith(("pretrained.", "scratch.")) and not never(k)]
    if frozen:
        keys = [k for k in keys if not k.startswith("pretrained.model.")]
    return types.SimpleNamespace(grads={k: None for k in keys}, frozen_encoder=frozen)


@pytest.mark.parametrize("make", [_seg_module, _zs_module], ids=["LSegmentationModule", "LSegModuleZS"])
def test_midasproto_returns_engine_adam_with_the_reference_groups(make):
    from modules.lsegmentation_module import EngineAdam, EngineSGD
    m = make(midasproto=True)
    (opt,), (sch,) = m.configure_optimizers()
    assert isinstance(opt, EngineAdam) and isinstance(opt, torch.optim.Adam) and not isinstance(opt, torch.optim.SGD)
    assert isinstance(sch, torch.optim.lr_scheduler.LambdaLR)
    g = opt._live_groups()
    assert len(g) == 2
    assert [x["lr"] for x in g] == pytest.approx([m.base_lr, 10 * m.base_lr])
    assert _ids(g[0]["params"]) == _ids(m.net.pretrained.parameters()) and _ids(g[1]["params"]) == _ids(m.net.scratch.parameters())
    assert all(tuple(x["betas"]) == (0.9, 0.999) and x["weight_decay"] == 1e-4 and x["eps"] == 1e-8 and not x["amsgrad"] for x in g)
    assert opt._fusable() and opt._fusable(_stub_engine(m.net, frozen=False))
    # without the flag nothing changes: SGD, momentum 0.9
    (sgd,), _ = make().configure_optimizers()
    assert isinstance(sgd, EngineSGD) and isinstance(sgd, torch.optim.SGD) and sgd.param_groups[0]["momentum"] == 0.9
    (sgd,), _ = make(midasproto=False).configure_optimizers()
    assert isinstance(sgd, EngineSGD)


def test_engine_adam_without_an_engine_is_torch_adam_and_round_trips_checkpoints():
    from modules.lsegmentation_module import EngineAdam
    g = torch.Generator().manual_seed(0)
    w0 = [torch.randn(5, 3, generator=g), torch.randn(7, generator=g)]
    grads = [[torch.randn_like(w, generator=None) for w in w0] for _ in range(3)]
    kw = dict(lr=1e-2, betas=(0.9, 0.999), weight_decay=1e-4)

    def make(cls, **extra):
        ps = [torch.nn.Parameter(w.clone()) for w in w0]
        return ps, cls([{"params": [ps[0]], "lr": 1e-3}, {"params": [ps[1]]}], **kw, **extra)

    pa, a = make(EngineAdam, net=None)
    pb, b = make(torch.optim.Adam)
    for step in range(2):
        for ps in (pa, pb):
            for p, gr in zip(ps, grads[step]):
                p.grad = gr.clone()
        a.step(); b.step()
    assert all(torch.equal(x, y) for x, y in zip(pa, pb))
    # EngineAdam -> plain Adam -> EngineAdam, then one more step on each: still the same numbers
    pc, c = make(torch.optim.Adam)
    c.load_state_dict(copy.deepcopy(a.state_dict()))          # (torch's load_state_dict may keep the tensors it is given)
    pd, d = make(EngineAdam, net=None)
    d.load_state_dict(copy.deepcopy(b.state_dict()))
    for ps, src in ((pc, pa), (pd, pb)):
        for p, q in zip(ps, src):
            p.data.copy_(q.data)
    for ps in (pa, pc, pd):
        for p, gr in zip(ps, grads[2]):
            p.grad = gr.clone()
    a.step(); c.step(); d.step()
    assert all(torch.equal(x, y) and torch.equal(x, z) for x, y, z in zip(pa, pc, pd))
    assert int(a.state[pa[0]]["step"]) == int(c.state[pc[0]]["step"]) == int(d.state[pd[0]]["step"]) == 3
    assert set(a.state_dict()["state"][0]) == {"step", "exp_avg", "exp_avg_sq"}


@pytest.mark.parametrize("midas", [False, True], ids=["sgd", "adam"])
def test_clip_fixed_layout_is_fusable_only_on_a_frozen_encoder_engine(midas):
    m = _zs_module(use_pretrained="clip_fixed", skip_frozen_backward=True, midasproto=midas)
    assert m.fixed_encoder and m.skip_frozen_backward and m.net.freeze_encoder
    (opt,), _ = m.configure_optimizers()
    g = opt.param_groups
    assert len(g) == 7 and [x["lr"] for x in g] == pytest.approx([0.0] + [m.base_lr] * 4 + [10 * m.base_lr] * 2)     # the reference's groups
    frozen, plain = _stub_engine(m.net, True), _stub_engine(m.net, False)
    assert opt._fusable(frozen)
    assert not opt._fusable(plain) and not opt._fusable()                  # as before on a non-frozen engine / with no engine
    assert opt._step_lrs(opt._live_groups()) == (m.base_lr, 10 * m.base_lr)
    # the encoder group must sit at lr 0 and the four act_postprocess groups at one lr
    g[0]["lr"] = 1e-3
    assert not opt._fusable(frozen)
    g[0]["lr"] = 0
    g[2]["lr"] = 2 * m.base_lr
    assert not opt._fusable(frozen)
    g[2]["lr"] = m.base_lr
    assert opt._fusable(frozen)
    # a tensor frozen by hand sends the step to torch; unequal hyper-parameters too
    p = g[5]["params"][0]
    p.requires_grad_(False)
    assert not opt._fusable(frozen)
    p.requires_grad_(True)
    g[5]["weight_decay"] = 0.0
    assert not opt._fusable(frozen)


def test_skip_frozen_backward_needs_clip_fixed_and_defaults_off():
    assert not _zs_module(use_pretrained="clip_fixed").net.freeze_encoder
    m = _zs_module(use_pretrained="False", skip_frozen_backward=True)
    assert not m.skip_frozen_backward and not m.net.freeze_encoder
    (opt,), _ = m.configure_optimizers()
    assert opt._fusable(_stub_engine(m.net, False))
    # the two-group layout on a frozen-encoder engine would leave pretrained.model.* to nobody: torch's step
    assert not opt._fusable(_stub_engine(m.net, True))


def test_engine_adam_refuses_what_the_kernel_does_not_implement():
    from modules.lsegmentation_module import EngineAdam
    a, b = (torch.nn.Parameter(torch.zeros(3)) for _ in range(2))
    groups = lambda: [{"params": [a]}, {"params": [b]}]
    assert EngineAdam(groups(), lr=0.1)._fusable()
    assert EngineAdam(groups() + [{"params": []}], lr=0.1)._fusable()
    assert not EngineAdam(groups(), lr=0.1, amsgrad=True)._fusable()
    assert not EngineAdam(groups(), lr=0.1, maximize=True)._fusable()
    assert not EngineAdam([{"params": [a], "betas": (0.8, 0.999)}, {"params": [b]}], lr=0.1)._fusable()
    assert not EngineAdam([{"params": [a], "eps": 1e-6}, {"params": [b]}], lr=0.1)._fusable()
    assert not EngineAdam([{"params": [a], "weight_decay": 0.1}, {"params": [b]}], lr=0.1)._fusable()
    assert not EngineAdam([{"params": [a]}], lr=0.1)._fusable()


def test_new_entry_points_are_declared_exported_and_bound(repo_root):
    from lseg_hip import _lib
    lib = _lib.load()
    hdr = open(os.path.join(repo_root, "include", "lseg_hip.h")).read()
    for name, arity in NEW_SYMBOLS.items():
        m = re.search(r"^int\s+" + name + r"\s*\(([^;]*)\)\s*;", hdr, re.M | re.S)
        assert m, f"{name} is not declared in include/lseg_hip.h"
        args = re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S)
        assert len([a for a in args.split(",") if a.strip()]) == arity, (name, args)
        assert hasattr(lib, name), f"{name} is not exported by the built library"
        assert name in _lib.SIGNATURES and len(_lib.SIGNATURES[name][1]) == arity, name
    # each declaration cites the reference lines it replaces
    doc = hdr.split("/* ---- training step")[1]
    assert "lsegmentation_module.py:152-163" in doc and "lsegmentation_module_zs.py:270-281" in doc and "lsegmentation_module_zs.py:220-235" in doc
