"""The fused Adam step (lseg_adam_step, csrc/elementwise.hip adam_multi_kernel) -- the --midasproto optimizer of the reference
(modules/lsegmentation_module.py:152-163, modules/lsegmentation_module_zs.py:270-281) -- on the engine and through EngineAdam:

  * three steps against an fp64 restatement of torch.optim.Adam on the same fp32 gradients and masters, held to 4 x the error CPU
    torch.optim.Adam in fp32 shows against the same oracle (parameter change, exp_avg, exp_avg_sq; weight decay 1e-4 and 0);
  * lr = 0 leaves the masters bit-unchanged while exp_avg / exp_avg_sq move;
  * the operand copies the kernel writes ARE the re-pack: an eval forward equals a fresh engine's on the updated masters, bit for bit;
  * LSegModuleZS(midasproto=True): the fused step runs, a hand-frozen tensor sends the next step to torch with the state carried over;
  * checkpoints: EngineAdam -> torch.optim.Adam -> EngineAdam, the restored fused step bit-identical to an uninterrupted run.

tiny16 at 64 x 64, B = 2, synthetic weights, bf16 operands, deterministic reductions: parameters with n % 4 != 0 (scalar path), larger
than one 4096-element chunk, with and without a 16-bit / fp32 copy.
"""
import copy

import pytest
import torch

pytestmark = pytest.mark.gpu

from lseg_hip.engine import HipEngine                                             # noqa: E402
from optim_helpers import (BETAS, EPS, LRS, adam_errors, make_batch, train_step, trained_engine, zs_module)      # noqa: E402

# ---- 1. the engine against fp64 ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("wd,head_blocks", [(1e-4, False), (0.0, False), (1e-4, True)], ids=["wd1e-4", "wd0", "wd1e-4-scalar-path"])
def test_fused_adam_matches_fp64_within_four_times_torch_fp32(wd, head_blocks):
    """Measured (MI355X, tiny16, 3 steps), worst per-tensor error against fp64 as engine / CPU torch fp32:
    weight decay 1e-4: parameter change 1.51e-05 / 1.51e-05, exp_avg 5.35e-08 / 5.23e-08, exp_avg_sq 1.27e-07 / 1.27e-07;
    weight decay 0: parameter change 1.67e-05 / 1.67e-05, exp_avg 5.5e-08 / 5.68e-08, exp_avg_sq 1.12e-07 / 1.12e-07;
    weight decay 1e-4, scalar path: parameter change 1.56e-05 / 1.56e-05, exp_avg 1.63e-07 / 2.53e-07, exp_avg_sq 1.04e-07 / 1.04e-07."""
    eng, sd, _, _ = trained_engine(head_blocks=head_blocks)
    keys = sorted(eng.grads)
    assert any(eng.grads[k].numel() > 4096 for k in keys)
    # the vectorised path needs 16-byte aligned masters and gradients and n % 4 == 0; the plain net has only such parameters
    scalar = [k for k in keys if eng.grads[k].numel() % 4 or (eng.grads[k].data_ptr() | eng.bound[k].data_ptr()) % 16]
    if head_blocks:
        assert any(eng.grads[k].numel() % 4 for k in scalar) and any(eng.grads[k].numel() > 4096 for k in scalar) and len(scalar) < len(keys)
    else:
        assert not scalar
    grads = {k: eng.grads[k].clone() for k in keys}
    w0 = {k: eng.bound[k].clone() for k in keys}
    for t, (lp, ls) in enumerate(LRS):
        eng.adam_step(lp, ls, t + 1, betas=BETAS, eps=EPS, weight_decay=wd)
    torch.cuda.synchronize()
    got = {k: (eng.bound[k].clone(),) + eng.get_adam_state(k) for k in keys}
    torch.cuda.synchronize()
    lrs_of = lambda k: [p[1] if k.startswith("scratch.") else p[0] for p in LRS]
    worst = adam_errors(w0, grads, lrs_of, wd, got)
    for i, what in enumerate(("parameter change", "exp_avg", "exp_avg_sq")):
        print(f"weight decay {wd:g}: {what}: engine {worst['engine'][i]:.3g}, CPU torch fp32 {worst['torch'][i]:.3g} (bar 4 x)")
    for i, what in enumerate(("parameter change", "exp_avg", "exp_avg_sq")):
        assert worst["engine"][i] <= 4 * worst["torch"][i], (what, worst)
    eng.close()


# ---- 2. lr = 0 --------------------------------------------------------------------------------------------------------------------------
def test_lr_zero_moves_the_moments_and_not_the_masters():
    eng, sd, _, _ = trained_engine()
    keys = sorted(eng.grads)
    w0 = {k: eng.bound[k].clone() for k in keys}
    eng.adam_step(0.0, 0.0, 1, betas=BETAS, eps=EPS, weight_decay=1e-4)
    torch.cuda.synchronize()
    assert all(torch.equal(eng.bound[k], w0[k]) for k in keys)
    for k in keys:
        m, v = eng.get_adam_state(k)
        torch.cuda.synchronize()
        if eng.grads[k].abs().max() > 0:
            assert m.abs().max() > 0 and v.abs().max() > 0, k
    # ... one group at lr 0, the other moving
    eng.adam_step(0.0, 1e-2, 2, betas=BETAS, eps=EPS, weight_decay=1e-4)
    torch.cuda.synchronize()
    assert all(torch.equal(eng.bound[k], w0[k]) for k in keys if k.startswith("pretrained."))
    assert not torch.equal(eng.bound["scratch.head1.weight"], w0["scratch.head1.weight"])
    eng.close()


# ---- 3. the operand copies ------------------------------------------------------------------------------------------------------------
def test_operand_copies_written_by_the_kernel_are_the_repack():
    eng, sd, x, tok = trained_engine()
    before = eng.bound["pretrained.model.blocks.0.attn.qkv.weight"].clone()
    eng.adam_step(1e-3, 1e-2, 1, betas=BETAS, eps=EPS, weight_decay=1e-4)
    eng.adam_step(1e-3, 1e-2, 2, betas=BETAS, eps=EPS, weight_decay=1e-4)
    torch.cuda.synchronize()
    assert not torch.equal(before, eng.bound["pretrained.model.blocks.0.attn.qkv.weight"])
    eng.set_train(False)
    out_a = eng.forward(x).clone()
    fresh = HipEngine(eng.cfg, 64, 64, max_batch=2, max_labels=4, deterministic=True)
    fresh.load_state_dict({k: v.detach().clone() for k, v in eng.bound.items()})
    fresh.set_tokens(tok, labels_per_image=2)
    out_b = fresh.forward(x)
    torch.cuda.synchronize()
    assert torch.isfinite(out_a).all() and torch.equal(out_a, out_b), (out_a - out_b).abs().max().item()
    eng.close(); fresh.close()


# ---- 4. / 5. the module path ------------------------------------------------------------------------------------------------------------
def test_module_path_runs_the_fused_step_and_hands_the_state_to_torch(monkeypatch):
    from modules.lsegmentation_module import EngineAdam
    m = zs_module(use_pretrained="False", midasproto=True)
    (opt,), _ = m.configure_optimizers()
    assert isinstance(opt, EngineAdam)
    named = dict(m.net.named_parameters())
    before = {k: p.detach().clone() for k, p in named.items()}
    batch = make_batch()
    train_step(m, opt, batch)
    eng = next(e for e in m.net._engines.values() if getattr(e, "_ts", None) is not None)
    assert eng._ts.adam_steps == 1 and eng._ts.sgd_steps == 0 and not opt.state                 # the engine's fused lseg_adam_step ran
    for k in ("scratch.head1.weight", "pretrained.model.blocks.1.mlp.fc1.weight", "pretrained.act_postprocess2.3.weight"):
        assert not torch.equal(named[k].detach(), before[k]), k
    # a tensor frozen by hand: the next step is torch's, on the engine's state
    held = {k: eng.get_adam_state(k) for k in eng.grads}
    torch.cuda.synchronize()
    seen = {}
    torch_step = torch.optim.Adam.step

    def spy(self, *a, **kw):
        seen.update({k: (int(self.state[p]["step"]), self.state[p]["exp_avg"].clone(), self.state[p]["exp_avg_sq"].clone())
                     for k, p in named.items() if p in self.state})
        return torch_step(self, *a, **kw)

    monkeypatch.setattr(torch.optim.Adam, "step", spy)
    named["scratch.head1.bias"].requires_grad_(False)
    train_step(m, opt, batch)
    assert eng._ts.adam_steps == 0 and set(seen) == set(held)
    for k, (step, ea, eas) in seen.items():
        assert step == 1 and torch.equal(ea, held[k][0]) and torch.equal(eas, held[k][1]), k
    assert int(opt.state[named["scratch.head1.weight"]]["step"]) == 2
    # ... and back: trainable again, the fused step takes torch's state over
    named["scratch.head1.bias"].requires_grad_(True)
    train_step(m, opt, batch)
    assert eng._ts.adam_steps == 3 and not opt.state


def test_checkpoint_round_trips_with_plain_torch_adam():
    batch = make_batch()
    # an uninterrupted run: two fused steps
    ref = zs_module(use_pretrained="False", midasproto=True)
    (ropt,), _ = ref.configure_optimizers()
    train_step(ref, ropt, batch)
    train_step(ref, ropt, batch)
    # the same run with the optimizer state taken through a plain torch.optim.Adam between the steps
    m = zs_module(use_pretrained="False", midasproto=True)
    (opt,), _ = m.configure_optimizers()
    train_step(m, opt, batch)
    eng = next(e for e in m.net._engines.values() if getattr(e, "_ts", None) is not None)
    named = dict(m.net.named_parameters())
    plain = torch.optim.Adam([{"params": list(g["params"]), "lr": g["lr"]} for g in opt.param_groups], lr=m.base_lr, betas=BETAS,
                             weight_decay=1e-4)
    plain.load_state_dict(copy.deepcopy(opt.state_dict()))
    for k in ("scratch.head1.weight", "pretrained.model.blocks.0.norm1.bias", "pretrained.act_postprocess1.4.weight"):
        st, (ea, eas) = plain.state[named[k]], eng.get_adam_state(k)
        torch.cuda.synchronize()
        assert int(st["step"]) == 1 and torch.equal(st["exp_avg"], ea) and torch.equal(st["exp_avg_sq"], eas), k
    (opt2,), _ = m.configure_optimizers()
    opt2.load_state_dict(copy.deepcopy(plain.state_dict()))
    train_step(m, opt2, batch)
    assert eng._ts.adam_steps == 2
    rn = dict(ref.net.named_parameters())
    diff = [k for k in named if not torch.equal(named[k].detach(), rn[k].detach())]
    assert not diff, diff[:5]
