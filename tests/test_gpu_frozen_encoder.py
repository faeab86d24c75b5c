"""Frozen-encoder training (lseg_set_frozen_encoder; the reference's use_pretrained='clip_fixed' puts pretrained.model at lr 0,
modules/lsegmentation_module_zs.py:220-235, and still pays the whole ViT backward):

  * a frozen and an unfrozen engine on the same inputs: logits, loss and every pretrained.act_postprocess* / scratch.* gradient are
    bit-identical (those gradients do not depend on the skipped part) -- fused loss, d(logits) hand-over, accumulation;
  * pretrained.model.* has no bucket, every bucket callback still fires once and in order, the step is deterministic;
  * LSegModuleZS(use_pretrained='clip_fixed', skip_frozen_backward=True) takes the fused SGD / Adam step on the reference's six groups
    and lands where the default clip_fixed path (full backward + torch's step) lands;
  * the refusals.

tiny16 at 64 x 64, B = 2, synthetic weights, bf16 operands, deterministic reductions.
"""
import ctypes as C
import warnings

import pytest
import torch

pytestmark = pytest.mark.gpu

from lseg_hip import _lib                                                         # noqa: E402
from lseg_hip.config import get_config                                            # noqa: E402
from lseg_hip.engine import HipEngine                                             # noqa: E402
from lseg_hip.synth import synthetic_state_dict, synthetic_tokens, synthetic_images   # noqa: E402
from train_helpers import rel                                                     # noqa: E402
from optim_helpers import adam_fp64, adam_torch_cpu, err, make_batch, make_target, pair_tokens                       # noqa: E402

TRAINED = ("pretrained.act_postprocess", "scratch.")


def _engine(freeze, seed=31):
    cfg = get_config("tiny16")
    sd = {k: v.cuda() for k, v in synthetic_state_dict(cfg, seed=seed).items()}
    eng = HipEngine(cfg, 64, 64, max_batch=2, max_labels=4, deterministic=True)
    eng.load_state_dict(sd)
    eng.set_tokens(pair_tokens(cfg, [2, 6]), labels_per_image=2)
    eng.enable_training(sd, freeze_encoder=freeze)
    return eng


@pytest.fixture(scope="module")
def pair():
    a, b = _engine(True), _engine(False)
    yield a, b
    a.close(); b.close()


# ---- 1. same inputs, frozen and unfrozen ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["fused_loss", "dlogits"])
def test_frozen_engine_computes_the_unfrozen_logits_loss_and_head_gradients(pair, mode):
    fz, un = pair
    x = synthetic_images(2, 64, 64, seed=31).cuda()
    target = make_target(2, 64, 64, 31).cuda()
    dl = (torch.randn((2, 2, 64, 64), generator=torch.Generator().manual_seed(3)) * 1e-3).cuda()
    res = []
    for eng in (fz, un):
        out = eng.forward(x).clone()
        loss = eng.backward(target=target, ignore_index=-100) if mode == "fused_loss" else eng.backward(dlogits=dl)
        torch.cuda.synchronize()
        res.append((out, None if loss is None else loss.clone(), {k: v.clone() for k, v in eng.grads.items()}))
    (out_f, loss_f, g_f), (out_u, loss_u, g_u) = res
    assert torch.equal(out_f, out_u)
    if mode == "fused_loss":
        assert torch.equal(loss_f, loss_u)
    want = {k for k in g_u if k.startswith(TRAINED)}
    assert want and set(g_f) == want and not [k for k in g_f if k.startswith("pretrained.model.")]
    assert not [k for k in want if not torch.equal(g_f[k], g_u[k])]
    assert all(g_f[k].abs().max() > 0 for k in ("pretrained.act_postprocess1.0.project.0.weight", "pretrained.act_postprocess4.0.project.0.bias",
                                                "scratch.head1.weight"))
    # accumulate_grad_batches: a second backward adds the same gradient (the bar of tests/test_gpu_train_zs.py)
    if mode == "fused_loss":
        fz.backward(target=target, ignore_index=-100, accumulate=True)
    else:
        fz.backward(dlogits=dl, accumulate=True)
    torch.cuda.synchronize()
    assert max(rel(fz.grads[k], 2 * g_f[k]) for k in g_f) <= 1e-2


# ---- 2. frozen keys, buckets, determinism ---------------------------------------------------------------------------------------------
def test_frozen_keys_have_no_bucket_and_every_bucket_still_fires_once_in_order(pair):
    fz, un = pair
    lib = fz.lib
    for k in fz.bound:
        b_f, b_u = lib.lseg_grad_bucket(fz._h, k.encode()), lib.lseg_grad_bucket(un._h, k.encode())
        if k.startswith("pretrained.model."):
            assert b_f == -1, k
        else:
            assert b_f == b_u, k                                   # the readouts and the reassemble keep their bucket indices
    assert lib.lseg_num_grad_buckets(fz._h) == lib.lseg_num_grad_buckets(un._h) == len(fz.grad_buckets)
    p, n = C.c_void_p(), C.c_size_t(0)
    assert lib.lseg_grad_ptr(fz._h, b"pretrained.model.blocks.0.attn.qkv.weight", C.byref(p), C.byref(n)) == -4      # no gradient buffer
    assert lib.lseg_adam_state(fz._h, b"pretrained.model.blocks.0.attn.qkv.weight", 0, C.byref(p), C.byref(n)) == -6  # no Adam state
    assert lib.lseg_sgd_momentum(fz._h, b"pretrained.model.cls_token", C.byref(p), C.byref(n)) == -6                  # no momentum
    x = synthetic_images(2, 64, 64, seed=32).cuda()
    target = make_target(2, 64, 64, 32).cuda()
    seen, runs = [], []
    fz.set_bucket_callback(lambda b: seen.append(b))
    for _ in range(2):
        out = fz.forward(x).clone()
        loss = fz.backward(target=target, ignore_index=-100)
        torch.cuda.synchronize()
        runs.append((out, loss.clone(), {k: v.clone() for k, v in fz.grads.items()}))
    fz.set_bucket_callback(None)
    nb = len(fz.grad_buckets)
    assert seen == list(range(nb)) * 2
    assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1])
    assert not [k for k in runs[0][2] if not torch.equal(runs[0][2][k], runs[1][2][k])]


# ---- 3. the module path -----------------------------------------------------------------------------------------------------------------
def _zs_module(seed=13, **kw):
    warnings.simplefilter("ignore")
    from modules.lseg_module_zs import LSegModuleZS
    m = LSegModuleZS("nowhere", "fss", 2, 0.004, 10, backbone="tiny16", num_features=64, arch_option=0, block_depth=0,
                     activation="lrelu", aux=False, weight_decay=1e-4, finetune_mode=True, nshot=1, use_pretrained="clip_fixed", **kw)
    m.net.load_state_dict(synthetic_state_dict(get_config("tiny16"), seed=seed))
    m.net.cuda().train()
    return m


@pytest.mark.parametrize("midas", [False, True], ids=["sgd", "adam"])
def test_skip_frozen_backward_module_takes_the_fused_step_and_lands_on_the_default_path(midas):
    """Adam, measured (MI355X): worst parameter-change error 1.49e-06 (14 of 78 tensors bit-identical), bar 4 x 6.16e-06."""
    batch = make_batch(13)
    m = _zs_module(skip_frozen_backward=True, midasproto=midas)
    twin = _zs_module(midasproto=midas)                                          # the default clip_fixed path: full backward + torch's step
    named, tnamed = dict(m.net.named_parameters()), dict(twin.net.named_parameters())
    before = {k: p.detach().clone() for k, p in named.items()}
    (opt,), _ = m.configure_optimizers()
    (topt,), _ = twin.configure_optimizers()
    assert len(opt.param_groups) == 7 and opt.param_groups[0]["lr"] == 0            # the reference's six groups (+ the empty auxlayer one)
    for mod, o in ((m, opt), (twin, topt)):
        o.zero_grad()
        mod.training_step(batch, 0).backward()
    eng, teng = opt._engine(), topt._engine()
    assert eng.frozen_encoder and not teng.frozen_encoder
    frozen = [k for k in named if k.startswith("pretrained.model.")]
    assert frozen and all(named[k].grad is None for k in frozen)
    assert tnamed["pretrained.model.blocks.0.attn.qkv.weight"].grad is not None
    assert opt._fusable(eng) and not topt._fusable(teng)
    tgrads = {k: tnamed[k].grad.clone() for k in eng.grads}
    opt.step(); topt.step()
    torch.cuda.synchronize()
    ts = eng._ts
    assert (ts.adam_steps, ts.sgd_steps) == ((1, 0) if midas else (0, 1))          # the fused step ran
    assert (teng._ts.adam_steps, teng._ts.sgd_steps) == (0, 0)
    assert all(torch.equal(named[k].detach(), before[k]) for k in frozen)
    moved = [k for k in named if k.startswith(TRAINED) and named[k].grad is not None]
    assert set(moved) == set(eng.grads) and all(not torch.equal(named[k].detach(), before[k]) for k in moved)
    if not midas:
        # the bar of tests/test_gpu_train.py::test_fused_sgd_matches_torch_sgd
        for k in moved:
            assert torch.allclose(named[k].detach(), tnamed[k].detach(), rtol=1e-5, atol=1e-7), k
        return
    # Adam: the bar of tests/test_gpu_adam.py -- 4 x the error CPU torch.optim.Adam in fp32 shows against fp64 on these gradients
    lr_of = lambda k: [m.base_lr * 10 if k.startswith("scratch.") else m.base_lr]
    bar = worst = 0.0
    for k in moved:
        ref = adam_fp64(before[k].cpu(), tgrads[k].cpu(), lr_of(k), 1e-4)[0]
        bar = max(bar, err(adam_torch_cpu(before[k], tgrads[k], lr_of(k), 1e-4)[0], ref, before[k]))
        worst = max(worst, err(named[k].detach(), tnamed[k].detach(), before[k]))
    same = sum(torch.equal(named[k].detach(), tnamed[k].detach()) for k in moved)
    print(f"frozen fused Adam against torch Adam on the twin: worst parameter-change error {worst:.3g} ({same} of {len(moved)} tensors "
          f"bit-identical), bar 4 x {bar:.3g}")
    assert worst <= 4 * bar, (worst, bar)


# ---- 4. refusals ----------------------------------------------------------------------------------------------------------------------
def test_frozen_encoder_refusals():
    cfg = get_config("tiny16")
    sd = {k: v.cuda() for k, v in synthetic_state_dict(cfg, seed=1).items()}
    eng = HipEngine(cfg, 64, 64, max_batch=1, max_labels=2)
    eng.load_state_dict(sd)
    eng.set_train(True)
    with pytest.raises(_lib.LSegError) as e:
        eng.set_frozen_encoder(True)
    assert e.value.code == -4                                                        # LSEG_ERR_STATE
    assert not eng.frozen_encoder
    eng.close()
    rn = HipEngine(get_config("clip_resnet101"), 64, 64, max_batch=1, max_labels=2, image_dtype="bf16")
    with pytest.raises(_lib.LSegError) as e:
        rn.set_frozen_encoder(True)
    assert e.value.code == -5                                                        # LSEG_ERR_UNSUPPORTED
    rn.close()
