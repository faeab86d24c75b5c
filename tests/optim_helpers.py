"""Shared helpers of the optimizer tests (tests/test_gpu_adam.py, tests/test_gpu_frozen_encoder.py): the tiny16 training engine after
one backward, torch.optim.Adam restated in fp64 and run through CPU torch in fp32, the error measure, and the zero-shot module with one
few-shot batch.  Test infrastructure only."""
import warnings

import torch

from lseg_hip.config import get_config
from lseg_hip.engine import HipEngine
from lseg_hip.synth import synthetic_state_dict, synthetic_tokens, synthetic_images

NAMES = ["others", "dog", "cat", "bird", "tree", "car", "boat", "cup", "lamp", "rock"]
BETAS, EPS = (0.9, 0.999), 1e-8
LRS = [(1e-3, 1e-2), (2e-3, 5e-3), (1e-3, 1e-2)]          # (pretrained.*, scratch.*) of the three steps


def make_target(B, H, W, seed):
    return torch.randint(0, 2, (B, H, W), generator=torch.Generator().manual_seed(2000 + seed))


def pair_tokens(cfg, ids):
    return torch.cat([synthetic_tokens(["others", NAMES[c]], cfg.text.vocab, cfg.text.ctx) for c in ids], 0)


def trained_engine(seed=21, head_blocks=False):
    """A training engine after one train-mode forward + backward: (engine, device state dict, x, tokens).  head_blocks: tiny16 with
    the arch_option 1 head block (shared labels) -- its 9-element weight and 1-element bias are the parameters with n % 4 != 0 -- and
    the gradient of the largest parameter re-bound to a view that is not 16-byte aligned: the kernel's scalar path, over several chunks."""
    cfg = get_config("tiny16", arch_option=1, block_depth=1) if head_blocks else get_config("tiny16")
    sd = {k: v.cuda() for k, v in synthetic_state_dict(cfg, seed=seed).items()}
    tok = synthetic_tokens(NAMES[:4], cfg.text.vocab, cfg.text.ctx) if head_blocks else pair_tokens(cfg, [3, 7])
    x = synthetic_images(2, 64, 64, seed=seed).cuda()
    eng = HipEngine(cfg, 64, 64, max_batch=2, max_labels=4, deterministic=True, head_block_training=head_blocks)
    eng.load_state_dict(sd)
    eng.set_tokens(tok, labels_per_image=0 if head_blocks else 2)
    eng.enable_training(sd)
    if head_blocks:
        import ctypes as C
        from lseg_hip import _lib
        k = max(eng.grads, key=lambda q: eng.grads[q].numel())
        flat = torch.zeros(eng.grads[k].numel() + 1, device="cuda")
        view = flat[1:].view(eng.grads[k].shape)
        _lib.check(eng.lib.lseg_bind_grad(eng._h, k.encode(), C.c_void_p(view.data_ptr())))
        eng.grads[k] = view
    eng.forward(x, want_logits=False)
    eng.backward(target=make_target(2, 64, 64, seed).cuda(), ignore_index=-100)
    torch.cuda.synchronize()
    return eng, sd, x, tok


def adam_fp64(w, g, lrs, wd, m=None, v=None, t0=0):
    """torch.optim.Adam (amsgrad / maximize off) restated in fp64 for one tensor: returns (w, exp_avg, exp_avg_sq) after len(lrs) steps."""
    w, g = w.double().clone(), g.double()
    m = torch.zeros_like(w) if m is None else m.double().clone()
    v = torch.zeros_like(w) if v is None else v.double().clone()
    for i, lr in enumerate(lrs):
        t = t0 + i + 1
        gg = g + wd * w
        m = BETAS[0] * m + (1 - BETAS[0]) * gg
        v = BETAS[1] * v + (1 - BETAS[1]) * gg * gg
        w = w - (lr / (1 - BETAS[0] ** t)) * m / (v.sqrt() / (1 - BETAS[1] ** t) ** 0.5 + EPS)
    return w, m, v


def adam_torch_cpu(w, g, lrs, wd):
    """The same steps through CPU torch.optim.Adam in fp32."""
    p = torch.nn.Parameter(w.float().cpu().clone())
    opt = torch.optim.Adam([p], lr=lrs[0], betas=BETAS, eps=EPS, weight_decay=wd)
    for lr in lrs:
        opt.param_groups[0]["lr"] = lr
        p.grad = g.float().cpu().clone()
        opt.step()
    return p.detach(), opt.state[p]["exp_avg"], opt.state[p]["exp_avg_sq"]


def err(got, ref, base=None):
    """relative error of `got` against the fp64 `ref` (of the CHANGE from `base` when given), norm over the tensor"""
    got, ref = got.double().cpu(), ref.double().cpu()
    if base is not None:
        got, ref = got - base.double().cpu(), ref - base.double().cpu()
    return ((got - ref).norm() / ref.norm().clamp_min(1e-300)).item()


def adam_errors(w0, grads, lrs_of, wd, got):
    """Worst per-tensor errors {dw, exp_avg, exp_avg_sq} against the fp64 oracle of (a) `got[k] = (w, m, v)` and (b) CPU torch Adam
    in fp32 on the same masters and gradients.  lrs_of(key) -> the learning rates of the steps."""
    worst = {"engine": [0.0, 0.0, 0.0], "torch": [0.0, 0.0, 0.0]}
    for k in grads:
        ref = adam_fp64(w0[k].cpu(), grads[k].cpu(), lrs_of(k), wd)
        for who, res in (("engine", got[k]), ("torch", adam_torch_cpu(w0[k], grads[k], lrs_of(k), wd))):
            e = (err(res[0], ref[0], w0[k]), err(res[1], ref[1]), err(res[2], ref[2]))
            worst[who] = [max(a, b) for a, b in zip(worst[who], e)]
    return worst


def zs_module(seed=9, **kw):
    warnings.simplefilter("ignore")
    from modules.lseg_module_zs import LSegModuleZS
    m = LSegModuleZS("nowhere", "fss", 2, 0.004, 10, backbone="tiny16", num_features=64, arch_option=0, block_depth=0,
                     activation="lrelu", aux=False, weight_decay=1e-4, finetune_mode=True, nshot=1, **kw)
    m.net.load_state_dict(synthetic_state_dict(get_config("tiny16"), seed=seed))
    m.net.cuda().train()
    return m


def make_batch(seed=9):
    return {"support_imgs": synthetic_images(2, 64, 64, seed=seed).view(2, 1, 3, 64, 64).cuda(),
            "support_masks": make_target(2, 64, 64, seed).view(2, 1, 64, 64).float().cuda(), "class_id": torch.tensor([4, 17]).cuda()}


def train_step(m, opt, batch):
    opt.zero_grad()
    loss = m.training_step(batch, 0)
    loss.backward()
    opt.step()
    torch.cuda.synchronize()
    return loss
