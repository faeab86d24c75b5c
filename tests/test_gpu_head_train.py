"""Training with the arch_option 1/2 head blocks (modules/models/lseg_net.py:43-79,198-201; csrc/head_train.hip; lseg_config.flags bit 4):

  * lseg_op_head_block_backward against fp64 autograd of oracle.lseg_oracle.head_block (both options, three activations, with and
    without the activation, odd shapes and K = 150), accumulation, the 16-bit row output = fp16 rounding of the planes, tie routing;
  * lseg_op_upsample_ce_backward_planes against fp64 autograd of cross_entropy(upsample_x2(low)) and against the rows op;
  * the whole step against oracle.training_step and against tests/golden/ref_head_train_*.pt (reference autograd);
  * determinism, accumulation, the d(logits) hand-over, the Python surface (LSegmentationModule + EngineSGD) and the refusals.
"""
import ctypes as C
import os
import types
import warnings

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

from lseg_hip import _lib                                                         # noqa: E402
from lseg_hip.config import get_config                                            # noqa: E402
from lseg_hip.engine import HipEngine                                             # noqa: E402
from lseg_hip.synth import synthetic_state_dict, synthetic_tokens, synthetic_images, read_labels   # noqa: E402
from oracle import make_golden as MG                                              # noqa: E402
from oracle.lseg_oracle import head_block, training_step                         # noqa: E402
from test_gpu_train import _compare_with_fixture, _violations                     # noqa: E402
from test_gpu_train_zs import _load_fixture                                       # noqa: E402  (unpacks the packed fixture schema)
from train_helpers import engine_step, rel, target_map                            # noqa: E402

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
HEAD_REF = sorted(f[:-3] for f in os.listdir(GOLD) if f.startswith("ref_head_train_"))
HB_W, HB_B = "scratch.head_block.depthwise.depthwise.weight", "scratch.head_block.depthwise.depthwise.bias"
ACTS = {"relu": 0, "lrelu": 1, "tanh": 2}
ERR_INVALID = -1                                  # LSEG_ERR_INVALID (include/lseg_hip.h)


def P(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def _st():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _op_bwd(x, y, dy, w9, bott, act, apply_act, dx_dtype=_lib.LSEG_F32, ldk=0, dW=None, db=None, accumulate=0, ws=None):
    B, K, H, W = x.shape
    lib = _lib.load()
    if dx_dtype == _lib.LSEG_F32:
        dx = torch.empty((B, K, H, W), dtype=torch.float32, device="cuda")
    else:
        dx = torch.full((B * H * W, ldk), float("nan"), dtype=torch.float16 if dx_dtype == _lib.LSEG_F16 else torch.bfloat16, device="cuda")
    dW = torch.zeros(9, device="cuda") if dW is None else dW
    db = torch.zeros(1, device="cuda") if db is None else db
    _lib.check(lib.lseg_op_head_block_backward(P(x), P(y), P(dy), P(w9), B, K, H, W, bott, ACTS[act], apply_act, P(dx), dx_dtype, ldk,
                                               P(dW), P(db), accumulate, P(ws), ws.numel() if ws is not None else 0, _st()))
    torch.cuda.synchronize()
    return dx, dW, db


def _ref_bwd(x, dy, w9, bias, bott, act, apply_act):
    """fp64 autograd of the oracle's head_block; also its fp32 output (the op's saved `out`)."""
    cfg = types.SimpleNamespace(arch_option=1 if bott else 2, activation=act)
    sd32 = {HB_W: w9.view(1, 1, 3, 3), HB_B: bias}
    y32 = head_block(sd32, cfg, x, apply_act)
    xd = x.double().requires_grad_(True)
    wd = w9.double().view(1, 1, 3, 3).requires_grad_(True)
    bd = bias.double().requires_grad_(True)
    yd = head_block({HB_W: wd, HB_B: bd}, cfg, xd, apply_act)
    yd.backward(dy.double())
    return y32, xd.grad, wd.grad.flatten(), bd.grad


def _case(B, K, H, W, seed, integer=False):
    g = torch.Generator().manual_seed(seed)
    x = torch.randint(-3, 4, (B, K, H, W), generator=g).float() if integer else torch.randn((B, K, H, W), generator=g) * 2
    dy = torch.randn((B, K, H, W), generator=g) * 1e-3
    w9 = torch.randn(9, generator=g) * 0.3
    bias = torch.randn(1, generator=g) * 0.05
    return x, dy, w9, bias


# ---- 1. one block: the op against fp64 autograd --------------------------------------------------------------------------------
# without the activation one activation name covers the K = 150 case
OP_CASES = [(bott, act, apply_act, shape) for bott in (1, 0) for act in ("relu", "lrelu", "tanh") for apply_act in (1, 0)
            for shape in ((2, 7, 13, 9), (1, 150, 60, 60)) if apply_act or act == "relu" or shape[1] != 150]


@pytest.mark.gpu_fast
@pytest.mark.parametrize("bott,act,apply_act,shape", OP_CASES)
def test_head_block_backward_op_matches_fp64_autograd(bott, act, apply_act, shape):
    B, K, H, W = shape
    x, dy, w9, bias = _case(B, K, H, W, seed=B * 1000 + K + H)
    y32, rdx, rdw, rdb = _ref_bwd(x, dy, w9, bias, bott, act, apply_act)
    dx, dW, db = _op_bwd(x.cuda(), y32.cuda(), dy.cuda(), w9.cuda(), bott, act, apply_act)
    assert rel(dx.cpu().double(), rdx) <= 1e-5, rel(dx.cpu().double(), rdx)
    assert rel(dW.cpu().double(), rdw) <= 1e-5 and rel(db.cpu().double(), rdb) <= 1e-5, (dW.cpu(), rdw, db.cpu(), rdb)
    # accumulate adds to the bound gradient
    dW2, db2 = dW.clone() + 1.0, db.clone() - 2.0
    base_w, base_b = dW2.clone(), db2.clone()
    _op_bwd(x.cuda(), y32.cuda(), dy.cuda(), w9.cuda(), bott, act, apply_act, dW=dW2, db=db2, accumulate=1)
    assert torch.equal(dW2, base_w + dW) and torch.equal(db2, base_b + db)
    # 16-bit rows (the correlation backward's operand): the fp16 rounding of the planes, transposed, zero padding columns
    ldk = (K + 63) // 64 * 64
    rows, _, _ = _op_bwd(x.cuda(), y32.cuda(), dy.cuda(), w9.cuda(), bott, act, apply_act, dx_dtype=_lib.LSEG_F16, ldk=ldk)
    want = dx.half().permute(0, 2, 3, 1).reshape(B * H * W, K)
    assert torch.equal(rows[:, :K], want)
    assert torch.equal(rows[:, K:], torch.zeros_like(rows[:, K:]))


def test_head_block_backward_with_a_caller_workspace_and_bf16_rows():
    x, dy, w9, bias = _case(2, 9, 17, 70, seed=5)
    y32, rdx, rdw, rdb = _ref_bwd(x, dy, w9, bias, 1, "lrelu", 1)
    lib = _lib.load()
    n = lib.lseg_op_head_block_backward_ws(2, 9, 17, 70, 1)
    ws = torch.empty(n, device="cuda")
    dx, dW, db = _op_bwd(x.cuda(), y32.cuda(), dy.cuda(), w9.cuda(), 1, "lrelu", 1, ws=ws)
    rows, dW2, db2 = _op_bwd(x.cuda(), y32.cuda(), dy.cuda(), w9.cuda(), 1, "lrelu", 1, dx_dtype=_lib.LSEG_BF16, ldk=16, ws=ws)
    assert rel(dx.cpu().double(), rdx) <= 1e-5
    assert torch.equal(rows[:, :9], dx.bfloat16().permute(0, 2, 3, 1).reshape(-1, 9))
    assert torch.equal(dW, dW2) and torch.equal(db, db2)


@pytest.mark.gpu_fast
def test_bottleneck_ties_route_to_the_first_maximal_label():
    # integer-valued planes in [-3, 3] over K = 12 labels: most pixels have several equal maxima
    x, dy, w9, bias = _case(2, 12, 16, 20, seed=11, integer=True)
    top = x.max(dim=1, keepdim=True)[0]
    assert ((x == top).sum(1) > 1).float().mean() > 0.3
    # torch CPU's own rule (the reference's): the gradient of max goes to the first maximal index
    probe = torch.tensor([[1.0, 3.0, 3.0, 2.0]], requires_grad=True)
    probe.max(dim=1)[0].sum().backward()
    assert probe.grad.tolist() == [[0.0, 1.0, 0.0, 0.0]]
    y32, rdx, rdw, rdb = _ref_bwd(x, dy, w9, bias, 1, "relu", 0)
    dx, dW, db = _op_bwd(x.cuda(), y32.cuda(), dy.cuda(), w9.cuda(), 1, "relu", 0)
    err = (dx.cpu().double() - rdx).abs().max().item()
    assert err <= 1e-6 * rdx.abs().max().item(), err


def test_head_block_backward_refuses_bad_arguments():
    lib = _lib.load()
    x = torch.zeros((1, 3, 4, 4), device="cuda")
    out = torch.zeros((16, 8), dtype=torch.float16, device="cuda")
    dW, db = torch.zeros(9, device="cuda"), torch.zeros(1, device="cuda")
    args = lambda **o: dict(dict(B=1, K=3, H=4, W=4, bott=1, act=0, apply_act=0, dt=_lib.LSEG_F16, ldk=8, y=None), **o)

    def call(a):
        return lib.lseg_op_head_block_backward(P(x), P(a["y"]), P(x), P(dW), a["B"], a["K"], a["H"], a["W"], a["bott"], a["act"], a["apply_act"],
                                               P(out), a["dt"], a["ldk"], P(dW), P(db), 0, None, 0, _st())
    assert call(args()) == 0
    assert call(args(ldk=4)) == ERR_INVALID            # ldk < K
    assert call(args(ldk=12)) == ERR_INVALID           # ldk % 8
    assert call(args(act=3)) == ERR_INVALID
    assert call(args(apply_act=1)) == ERR_INVALID      # the activation needs the saved output
    assert call(args(B=0)) == ERR_INVALID
    torch.cuda.synchronize()


# ---- 2. the fused CE backward as planes -------------------------------------------------------------------------------------------
@pytest.mark.gpu_fast
@pytest.mark.parametrize("B,K,h,w", [(2, 7, 13, 9), (1, 150, 60, 60)])
def test_upsample_ce_backward_planes_matches_fp64_and_the_rows_op(B, K, h, w):
    lib = _lib.load()
    g = torch.Generator().manual_seed(K + h)
    low = (torch.randn((B, K, h, w), generator=g) * 3).half().float()
    target = target_map(B, 2 * h, 2 * w, K, seed=K)
    ld = low.double().requires_grad_(True)
    F.cross_entropy(F.interpolate(ld, scale_factor=2, mode="bilinear", align_corners=True), target, ignore_index=-1).backward()
    planes = torch.empty((B, K, h, w), device="cuda")
    ksum = torch.empty((B, h, w), device="cuda")
    nll = torch.zeros(2, dtype=torch.float64, device="cuda")
    lse = torch.empty(B * 4 * h * w, device="cuda")
    lc, tc = low.cuda(), target.cuda()
    _lib.check(lib.lseg_op_upsample_ce_backward_planes(P(lc), P(tc), B, K, h, w, -1, P(nll), P(lse), P(planes), P(ksum), _st()))
    torch.cuda.synchronize()
    assert rel(planes.cpu().double(), ld.grad) <= 1e-4, rel(planes.cpu().double(), ld.grad)
    assert torch.allclose(ksum, planes.sum(1), rtol=1e-4, atol=1e-9)
    ldk = (K + 63) // 64 * 64
    rows = torch.empty((B * h * w, ldk), dtype=torch.float16, device="cuda")
    _lib.check(lib.lseg_op_upsample_ce_backward_rows(P(lc), P(tc), B, K, h, w, -1, P(nll), P(lse), P(rows), ldk, _lib.LSEG_F16, _st()))
    torch.cuda.synchronize()
    assert torch.equal(rows[:, :K], planes.half().permute(0, 2, 3, 1).reshape(-1, K))


# ---- 3. the whole step ----------------------------------------------------------------------------------------------------------
def _tiny(arch, depth, act, seed):
    cfg = get_config("tiny16", arch_option=arch, block_depth=depth, activation=act)
    return cfg, synthetic_state_dict(cfg, seed=seed)


@pytest.mark.parametrize("arch,depth,act", [(1, 0, "lrelu"), (1, 1, "relu"), (1, 2, "lrelu"), (1, 3, "tanh"),
                                            (2, 0, "relu"), (2, 2, "tanh"), (2, 3, "lrelu")])
def test_head_block_training_step_matches_the_oracle(arch, depth, act):
    cfg, sd = _tiny(arch, depth, act, seed=20 + 3 * depth + arch)
    B, H, W, K = 2, 64, 64, 5
    tok = synthetic_tokens(read_labels(MG.LABELS)[:K], cfg.text.vocab, cfg.text.ctx)
    x = synthetic_images(B, H, W, seed=depth)
    target = target_map(B, H, W, K, seed=depth)
    ref_loss, ref_grads = training_step(sd, x, target, tok, cfg, ignore_index=-1)
    eng, out, loss, _ = engine_step(cfg, sd, x, target, tok, head_block_training=True)
    assert abs(loss.item() - float(ref_loss)) <= 1e-2 * abs(float(ref_loss)), (loss.item(), float(ref_loss))
    trainable = {k for k in ref_grads if not k.startswith("clip_pretrained.")}
    assert set(eng.grads) == trainable, sorted(set(eng.grads) ^ trainable)[:10]
    # with a single block (depth 0 / 1) d(bias) = sum of d(out) = sum over pixels of sum_k (p_k - y_k) / n = 0: both sides hold rounding
    # noise, compared against the weight gradient's scale instead
    single = depth <= 1
    cmp = sorted(k for k in trainable if not (single and k == HB_B))
    report = {k: rel(eng.grads[k].cpu(), ref_grads[k]) for k in cmp}
    nerr = {k: abs(eng.grads[k].float().norm().item() - ref_grads[k].norm().item()) / ref_grads[k].norm().item() for k in cmp}
    scale = ref_grads[HB_W].norm().item()
    print(f"[arch {arch} depth {depth} {act}] loss {loss.item():.5f} vs {float(ref_loss):.5f}; max gradient error {max(report.values()):.4f}; "
          f"head block weight {report[HB_W]:.4f}, bias {float(eng.grads[HB_B]):.3e} vs {float(ref_grads[HB_B]):.3e} (|dW| {scale:.3e}); "
          f"max norm error {max(nerr.values()):.4f}")
    worst = sorted(report.items(), key=lambda kv: -kv[1])[:3]
    # bars from the measured table (MI355X): the loss within 0.03 %, the head-block weight gradient within 0.05-4.7 %; the tower's worst
    # tensors (cls_token, pos_embed, the first blocks' LayerNorm) at 0.37-0.51 and norm errors up to 0.33 -- above tests/test_gpu_train.py's
    # arch_option 0 bars (0.35 / 0.10): the bottleneck adds max_k to every logit and a block mixes 9 neighbours, so the bf16 forward's
    # logit noise reaches the softmax amplified (the d(logits)-given path below isolates the backward's own arithmetic)
    assert max(report.values()) <= 0.6 and max(nerr.values()) <= 0.4, worst
    assert sorted(report.values())[len(report) // 2] <= 0.35, worst         # depth 3: three activation masks, medians ~0.25-0.3
    assert report[HB_W] <= 0.05
    if single:
        assert abs(float(eng.grads[HB_B])) <= 1e-3 * scale and abs(float(ref_grads[HB_B])) <= 1e-3 * scale
    else:
        assert report[HB_B] <= 0.05


@pytest.mark.parametrize("name", [pytest.param(n, marks=pytest.mark.gpu_fast) if "_64x64_" in n else n for n in HEAD_REF])
def test_head_block_training_step_matches_fixtures_made_by_reference_autograd(name):
    g = _load_fixture(name)
    bb, H, W, B, K, arch, depth, act, seed = g["spec"]
    full = H >= 480
    cfg = get_config(bb, arch_option=arch, block_depth=depth, activation=act)
    sd = synthetic_state_dict(cfg, seed=seed)
    x = synthetic_images(B, H, W, seed=seed)
    eng, out, loss, _ = engine_step(cfg, sd, x, target_map(B, H, W, K, seed), g["tokens"], head_block_training=True)
    m = _compare_with_fixture(eng, g)
    med = lambda d: sorted(d.values())[len(d) // 2]
    print(f"{name}: loss {loss.item():.6f} vs {g['loss']:.6f}; norm error median {med(m['nerr']):.4f} worst {max(m['nerr'].values()):.4f}; "
          f"strided error median {med(m['serr']):.3f} worst {max(m['serr'].values()):.3f}; cosine median {med(m['cos']):.4f} "
          f"worst {min(m['cos'].values()):.4f}; head block norm error {m['nerr'][HB_W]:.4f} / {m['nerr'][HB_B]:.4f}")
    assert abs(loss.item() - g["loss"]) <= 1e-2 * abs(g["loss"]), (loss.item(), g["loss"])
    assert m["nerr"][HB_W] <= 0.05 and m["nerr"][HB_B] <= 0.05
    # the 480 x 480 fixture passes tests/test_gpu_train.py's bars unchanged (measured: cosine median 0.988, strided median 0.142); the small
    # crops relax the cosine median and the worst strided element as the zero-shot fixtures do (tests/test_gpu_train_zs.py: few pixels,
    # an fp16-subnormal head gradient).  Measured: ViT-L/16 64x64 cosine median 0.970, worst strided element 1.70; ViT-B/32 0.977 / 0.66.
    relaxed = {"median cosine": lambda v: v >= 0.96, "worst strided element error": lambda v: v <= 2.0}
    bad = [(k, v) for k, v in _violations(m, full) if full or k not in relaxed or not relaxed[k](v)]
    assert not bad, bad


def test_head_block_step_is_deterministic_accumulates_and_hands_over():
    cfg, sd = _tiny(1, 2, "lrelu", seed=31)
    B, H, W, K = 2, 64, 64, 5
    tok = synthetic_tokens(read_labels(MG.LABELS)[:K], cfg.text.vocab, cfg.text.ctx)
    x = synthetic_images(B, H, W, seed=31)
    target = target_map(B, H, W, K, seed=31)
    runs = []
    for _ in range(2):
        eng, out, loss, _ = engine_step(cfg, {k: v.clone() for k, v in sd.items()}, x, target, tok, head_block_training=True,
                                        deterministic=True)
        runs.append((out.clone(), float(loss), {k: v.clone() for k, v in eng.grads.items()}))
    assert torch.equal(runs[0][0], runs[1][0]) and runs[0][1] == runs[1][1]
    assert not [k for k in runs[0][2] if not torch.equal(runs[0][2][k], runs[1][2][k])]
    # every bucket callback fires (bucket 0 is enqueued after the head-block gradients: csrc/train.hip, Engine::backward)
    seen = []
    eng.set_bucket_callback(lambda b: seen.append(b))
    out = eng.forward(x.cuda())
    eng.backward(target=target.cuda(), ignore_index=-1)
    torch.cuda.synchronize()
    assert sorted(set(seen)) == list(range(len(eng.grad_buckets)))
    fused = {k: v.clone() for k, v in eng.grads.items()}
    assert all(torch.equal(fused[k], runs[0][2][k]) for k in fused)
    # accumulate_grad_batches: a second backward adds
    eng.backward(target=target.cuda(), ignore_index=-1, accumulate=True)
    torch.cuda.synchronize()
    assert max(rel(eng.grads[k], 2 * fused[k]) for k in fused) <= 1e-2
    assert rel(eng.grads[HB_W], 2 * fused[HB_W]) <= 1e-5
    # the d(logits) hand-over (autograd's d CE / d logits) equals the fused loss to rounding
    o = out.detach().clone().requires_grad_(True)
    F.cross_entropy(o, target.cuda(), ignore_index=-1).backward()
    eng.forward(x.cuda())
    eng.backward(dlogits=o.grad.contiguous())
    torch.cuda.synchronize()
    worst = max(rel(eng.grads[k], fused[k]) for k in fused)
    print(f"hand-over vs fused: worst {worst:.2e}, head block {rel(eng.grads[HB_W], fused[HB_W]):.2e}")
    assert worst <= 2e-2 and rel(eng.grads[HB_W], fused[HB_W]) <= 1e-3 and rel(eng.grads[HB_B], fused[HB_B]) <= 1e-3


# ---- 4. Python surface and refusals ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("arch", [1, 2])
def test_lsegnet_with_head_blocks_trains_through_the_module_and_engine_sgd(arch):
    warnings.simplefilter("ignore")
    from modules.lsegmentation_module import LSegmentationModule
    from modules.models.lseg_net import LSegNet
    cfg, sd = _tiny(arch, 2, "lrelu", seed=40 + arch)
    labels = read_labels(MG.LABELS)[:5]

    class M(LSegmentationModule):
        def __init__(self):
            super().__init__("", "ade20k", 16, 0.004, 10, ignore_index=-1, weight_decay=1e-4, se_loss=False, aux=False,
                             se_weight=0.2, aux_weight=0.2)
            self.nclass = self.num_classes = len(labels)
            self.net = LSegNet(labels=labels, backbone="tiny16", features=64, arch_option=arch, block_depth=2, activation="lrelu")
            self.criterion = torch.nn.CrossEntropyLoss(ignore_index=-1)

    m = M()
    m.net.load_state_dict(sd)
    m = m.cuda().train()
    (opt,), _ = m.configure_optimizers()
    assert type(opt).__name__ == "EngineSGD"
    named = dict(m.net.named_parameters())
    hb = [named[HB_W], named[HB_B]]
    grp = [g for g in opt.param_groups if any(p is hb[0] for p in g["params"])]
    assert len(grp) == 1 and all(any(p is q for q in grp[0]["params"]) for p in hb)
    x = synthetic_images(2, 64, 64, seed=arch).cuda()
    t = target_map(2, 64, 64, 5, seed=arch).cuda()
    loss = m.training_step((x, t), 0)
    loss.backward()
    assert all(p.grad is not None and float(p.grad.abs().sum()) > 0 for p in hb)
    eng = opt._engine()
    assert eng is not None and opt._fusable(eng)
    before = [p.detach().clone() for p in hb]
    grads = [p.grad.detach().clone() for p in hb]
    shadow = [b.clone().requires_grad_(True) for b in before]
    ref_opt = torch.optim.SGD(shadow, lr=grp[0]["lr"], momentum=grp[0]["momentum"], weight_decay=grp[0]["weight_decay"])
    for s, g in zip(shadow, grads):
        s.grad = g.clone()
    ref_opt.step()
    opt.step()
    torch.cuda.synchronize()
    assert eng._ts.sgd_steps == 1                                               # the fused lseg_sgd_step ran
    for p, b, s in zip(hb, before, shadow):
        assert not torch.equal(p.detach(), b)
        assert torch.allclose(p.detach(), s.detach(), rtol=1e-5, atol=1e-7), (p.detach(), s.detach())
    # the next step runs on the updated head block; eval still works
    opt.zero_grad()
    loss2 = m.training_step((x, t), 1)
    loss2.backward()
    assert torch.isfinite(loss2)
    m.net.eval()
    with torch.no_grad():
        ev = m.net(x)
    assert ev.shape == (2, 5, 64, 64) and torch.isfinite(ev).all()


def test_head_block_training_refusals():
    cfg, sd = _tiny(1, 2, "relu", seed=1)
    sdd = {k: v.cuda() for k, v in sd.items()}
    plain = HipEngine(cfg, 64, 64, max_batch=2, max_labels=4)                   # no flags bit 4
    plain.load_state_dict(sdd)
    with pytest.raises(_lib.LSegError, match="arch_option"):
        plain.set_train(True)
    plain.close()
    eng = HipEngine(cfg, 64, 64, max_batch=2, max_labels=4, head_block_training=True)
    eng.load_state_dict(sdd)
    eng.enable_training(sdd)
    eng.set_tokens(synthetic_tokens(["others", "dog", "others", "cat"], cfg.text.vocab, cfg.text.ctx), labels_per_image=2)
    with pytest.raises(_lib.LSegError, match="head blocks"):
        eng.forward(synthetic_images(2, 64, 64, seed=1).cuda())
    eng.close()
    fp16 = HipEngine(cfg, 64, 64, max_batch=1, max_labels=2, image_dtype="fp16", head_block_training=True)
    fp16.load_state_dict(sdd)
    with pytest.raises(_lib.LSegError, match="bf16"):
        fp16.set_train(True)
    fp16.close()
