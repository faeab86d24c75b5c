"""Few-shot episode evaluation on the device (csrc/episode.hip, lseg_op_episode_stats / lseg_episode_stats, HipEngine.episode_stats,
LSeg.evaluate_episode, LSegmentationModuleZS.validation_step):

  1. the bare kernel on full-resolution scores against the areas the REFERENCE'S OWN Evaluator recorded (tests/golden/ref_episode_*.pt);
  2. the low-resolution form (x2 bilinear on the fly) against tests/episode_helpers.py on lseg_op_upsample2x_planes of the same planes;
  3. determinism of the NLL, the meter scatter, NULL arguments, the flags;
  4. the refusals;
  5. the whole path on the tiny zero-shot networks (ViT and ResNet-101 tower);
  6. validation_step / validation_epoch_end and training_step with a train_average_meter.

The cross-entropy bar is tests/test_metrics.py's for the same fp32 exp / log arithmetic: 2e-5 * max(1, |ce|) of the fp64 value.
"""
import ctypes as C
import os
import warnings

import pytest
import torch
import torch.nn.functional as F

pytestmark = [pytest.mark.gpu, pytest.mark.gpu_fast]

import episode_helpers as eh                                                       # noqa: E402
from lseg_hip import _lib                                                          # noqa: E402
from lseg_hip.config import get_config                                             # noqa: E402
from lseg_hip.engine import HipEngine                                              # noqa: E402
from lseg_hip.episode import EpisodeMeter                                          # noqa: E402
from lseg_hip.synth import synthetic_state_dict, synthetic_tokens, synthetic_images  # noqa: E402

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
FIXTURES = sorted(f[:-3] for f in os.listdir(GOLD) if f.startswith("ref_episode_"))


def P(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def ce_bar(ref):
    return 2e-5 * max(1.0, abs(ref))


def op(scores, target, ignore=None, up=0, ignore_index=-100, class_id=None, nclass=0, inter_buf=None, union_buf=None):
    """lseg_op_episode_stats on device tensors -> (areas [B,6], nll [B,2], flags [2]); scores [B,2,H,W] or, up = 1, [B,2,H/2,W/2]."""
    lib = _lib.load()
    B, H, W = target.shape
    ws = torch.empty(max(1, lib.lseg_op_episode_stats_ws_bytes(B, H, W) // 8), dtype=torch.float64, device="cuda")
    areas = torch.full((B, 6), -7, dtype=torch.int64, device="cuda")               # overwritten, not accumulated
    nll = torch.full((B, 2), -7.0, dtype=torch.float64, device="cuda")
    flags = torch.full((2,), -7, dtype=torch.int64, device="cuda")
    _lib.check(lib.lseg_op_episode_stats(P(scores), P(target), P(ignore), B, H, W, up, ignore_index, P(class_id), nclass, P(inter_buf),
                                         P(union_buf), P(areas), P(nll), P(flags), P(ws), ws.numel() * 8, stream()))
    torch.cuda.synchronize()
    return areas.cpu(), nll.cpu(), flags.cpu()


# ---- 1. the kernel against the reference's Evaluator ------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", FIXTURES)
@pytest.mark.parametrize("tag", ["ignore", "noignore"])
def test_op_equals_the_reference_evaluator(name, tag):
    fx = torch.load(os.path.join(GOLD, name + ".pt"))
    scores, target, ignore = fx["scores_f16"].float(), fx["target_u8"].long(), fx["ignore_u8"]
    ig = ignore.cuda() if tag == "ignore" else None
    areas, nll, flags = op(scores.cuda(), target.cuda(), ig)
    inter, union = eh.inter_union(areas)
    print(name, tag, "areas", areas.tolist(), "nll", nll.tolist())
    assert torch.equal(inter, fx[f"area_inter_{tag}"]) and torch.equal(union, fx[f"area_union_{tag}"])
    assert torch.equal(areas, eh.classify(eh.predict(scores), target, ignore if tag == "ignore" else None))
    assert flags.tolist() == [0, 0]
    s, n = eh.cross_entropy(scores, target)                                        # the ignore mask does not enter the loss
    assert torch.equal(nll[:, 1], n)
    for b in range(scores.shape[0]):
        assert abs(float(nll[b, 0] / n[b]) - float(s[b] / n[b])) <= ce_bar(float(s[b] / n[b]))


@pytest.mark.parametrize("H,W,B", [(9, 11, 3), (1, 1, 2), (7, 293, 2)])
def test_op_on_odd_sizes_and_unaligned_targets(H, W, B):
    """H * W odd: every second image's target row starts off a 16-byte boundary (scalar head / tail around the 16-byte loads), and a
    target tensor that itself starts 8 bytes off."""
    g = torch.Generator().manual_seed(H * W + B)
    scores = torch.randn(B, 2, H, W, generator=g)
    store = torch.randint(0, 2, (B * H * W + 1,), generator=g).cuda()
    ign = (torch.rand(B, H, W, generator=g) < 0.2)
    for off in (0, 1):
        target = store[off:off + B * H * W].view(B, H, W)
        assert target.data_ptr() % 16 == 8 * off
        t = target.cpu().clone()
        ig = (ign & (t == 0)).to(torch.uint8)
        areas, nll, flags = op(scores.cuda(), target, ig.cuda())
        assert torch.equal(areas, eh.classify(eh.predict(scores), t, ig)) and flags.tolist() == [0, 0]
        s, n = eh.cross_entropy(scores, t)
        assert torch.equal(nll[:, 1], n)
        assert abs(float(nll[:, 0].sum() / n.sum()) - float(s.sum() / n.sum())) <= ce_bar(float(s.sum() / n.sum()))


# ---- 2. through the x2 bilinear -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("h,w,B", [(5, 7, 3), (5, 8, 3), (48, 48, 2)])
def test_lowres_form_equals_the_materialised_logits(h, w, B):
    """The logits are materialised by lseg_op_upsample2x_planes where it takes the shape (it refuses W % 4 != 0: LSEG_ERR_UNSUPPORTED), and
    at 5 x 7 by lseg_op_eval_resize to (2h, 2w) -- the library's other materialising align_corners=True bilinear, the same src_tap / bilerp
    arithmetic on the same ratio (h - 1) / (2h - 1).  Equality is exact either way."""
    lib = _lib.load()
    g = torch.Generator().manual_seed(100 + h)
    low = (torch.randn(B, 2, h, w, generator=g) * 4).cuda()
    low[0, 1, : h // 2] = low[0, 0, : h // 2]                                      # ties that survive the interpolation
    H, W = 2 * h, 2 * w
    full = torch.empty(B, 2, H, W, device="cuda")
    if w % 4 == 0:
        _lib.check(lib.lseg_op_upsample2x_planes(P(low), P(full), B * 2, h, w, stream()))
    else:
        _lib.check(lib.lseg_op_eval_resize(P(low), P(full), B * 2, h, w, H, W, 0, stream()))
    target = torch.randint(0, 2, (B, H, W), generator=g)
    ignore = ((torch.rand(B, H, W, generator=g) < 0.1) & (target == 0)).to(torch.uint8)
    areas, nll, flags = op(low, target.cuda(), ignore.cuda(), up=1)
    fullc = full.cpu()
    ref = eh.classify(eh.predict(fullc), target, ignore)
    print(f"{h}x{w} B={B}: areas {areas.tolist()} ties {(fullc[:, 0] == fullc[:, 1]).sum().item()}")
    assert (fullc[:, 0] == fullc[:, 1]).sum().item() > 0
    assert torch.equal(areas, ref) and flags.tolist() == [0, 0]
    a0, n0, _ = op(full, target.cuda(), ignore.cuda(), up=0)                       # the same values -> the same bits
    assert torch.equal(a0, areas) and torch.equal(n0, nll)
    s, n = eh.cross_entropy(fullc, target)
    assert torch.equal(nll[:, 1], n)
    for b in range(B):
        ce = float(s[b] / n[b])
        print(f"  image {b}: ce kernel {float(nll[b, 0] / n[b]):.9f} fp64 {ce:.9f}")
        assert abs(float(nll[b, 0] / n[b]) - ce) <= ce_bar(ce)


# ---- 3. determinism, scatter, NULLs, flags --------------------------------------------------------------------------------------------------
def test_determinism_scatter_nulls_and_flags():
    g = torch.Generator().manual_seed(7)
    B, H, W, nclass = 4, 96, 96, 20
    scores = torch.randn(B, 2, H, W, generator=g).cuda()
    target = torch.randint(0, 2, (B, H, W), generator=g)
    ignore = ((torch.rand(B, H, W, generator=g) < 0.1) & (target == 0)).to(torch.uint8)
    ids = torch.tensor([3, 11, 3, 3])                                              # duplicates must add up
    ib = torch.zeros(2, nclass, dtype=torch.int64, device="cuda")
    ub = torch.zeros(2, nclass, dtype=torch.int64, device="cuda")
    a1, n1, f1 = op(scores, target.cuda(), ignore.cuda(), class_id=ids.cuda(), nclass=nclass, inter_buf=ib, union_buf=ub)
    a2, n2, f2 = op(scores, target.cuda(), ignore.cuda())                          # NULL meter buffers
    assert torch.equal(a1, a2) and torch.equal(n1, n2), "two calls on the same input must give the same bits"
    assert f1.tolist() == [0, 0] and f2.tolist() == [0, 0]
    inter, union = eh.inter_union(a1)
    ref_i = torch.zeros(2, nclass, dtype=torch.int64).index_add_(1, ids, inter)
    ref_u = torch.zeros(2, nclass, dtype=torch.int64).index_add_(1, ids, union)
    assert torch.equal(ib.cpu(), ref_i) and torch.equal(ub.cpu(), ref_u)
    op(scores, target.cuda(), ignore.cuda(), class_id=ids.cuda(), nclass=nclass, inter_buf=ib, union_buf=ub)   # the buffers accumulate
    assert torch.equal(ib.cpu(), 2 * ref_i) and torch.equal(ub.cpu(), 2 * ref_u)
    a3, n3, f3 = op(scores, target.cuda(), None)                                   # NULL ignore mask
    assert torch.equal(a3, eh.classify(eh.predict(scores.cpu()), target, None)) and torch.equal(n3, n1)
    # planted: 5 ignored pixels with target 1, 3 targets of 7, 2 of ignore_index
    t = target.clone()
    ig = ignore.clone()
    t[1, 0, :5] = 1
    ig[1, 0, :5] = 1
    t[2, 5, :3] = 7
    t[3, 9, :2] = -100
    a4, n4, f4 = op(scores, t.cuda(), ig.cuda())
    assert f4.tolist() == [5, 3] == eh.flags(t, ig).tolist()
    assert torch.equal(a4, eh.classify(eh.predict(scores.cpu()), t, ig))           # 7 is in no area_gt, the prediction still counts
    assert torch.equal(n4[:, 1], eh.cross_entropy(scores.cpu(), t)[1]) and int(n4[:, 1].sum()) == B * H * W - 5


# ---- 4. refusals ------------------------------------------------------------------------------------------------------------------------
def _tiny_engine(labels, per_image, B=2):
    cfg = get_config("tiny16")
    eng = HipEngine(cfg, 64, 64, max_batch=B, max_labels=len(labels), image_dtype="fp16")
    eng.load_state_dict(synthetic_state_dict(cfg, seed=5))
    eng.set_tokens(synthetic_tokens(labels, cfg.text.vocab, cfg.text.ctx), labels_per_image=per_image)
    return eng


def test_refusals():
    from test_gpu_corr_argmax import _tiny512_labels
    lib = _lib.load()
    t = torch.zeros(2, 64, 64, dtype=torch.int64, device="cuda")
    eng = _tiny_engine(["others", "cat", "others", "dog"], 2)
    with pytest.raises(_lib.LSegError) as e:                                       # before any forward
        eng.episode_stats(t)
    assert e.value.code == -4 and "no forward has run" in str(e.value)
    x = synthetic_images(2, 64, 64, seed=5).cuda()
    eng.forward(x, want_logits=False)
    meter = EpisodeMeter("pascal", range(20), "cuda")
    for ids in ([0, 20], [-1, 3], [1]):
        with pytest.raises(_lib.LSegError) as e:                                   # refused on the host, before the launch
            eng.episode_stats(t, class_id=ids, meter=meter)
        assert e.value.code == -1 and "nclass=20" in str(e.value)
    assert int(meter.intersection_buf.sum()) == 0 and int(meter.union_buf.sum()) == 0 and meter.loss_buf == []
    r = eng.episode_stats(t, class_id=[0, 19], meter=meter)
    assert int(r["areas"][:, 2:4].sum()) == 2 * 64 * 64
    eng.close()
    # the bare op: a half-given meter, a workspace too small
    areas = torch.zeros(2, 6, dtype=torch.int64, device="cuda")
    nll = torch.zeros(2, 2, dtype=torch.float64, device="cuda")
    flags = torch.zeros(2, dtype=torch.int64, device="cuda")
    ws = torch.zeros(64, dtype=torch.float64, device="cuda")
    s = torch.zeros(2, 2, 64, 64, device="cuda")
    assert lib.lseg_op_episode_stats(P(s), P(t), None, 2, 64, 64, 0, -100, P(t), 20, None, None, P(areas), P(nll), P(flags), P(ws), 512, stream()) == -1
    assert b"meter" in lib.lseg_last_error(None)
    assert lib.lseg_op_episode_stats(P(s), P(t), None, 2, 64, 64, 0, -100, None, 0, None, None, P(areas), P(nll), P(flags), P(ws), 8, stream()) == -1
    assert b"workspace" in lib.lseg_last_error(None)
    # after a K = 5 forward
    eng = _tiny_engine(["wall", "sky", "tree", "floor", "other"], 0)
    eng.forward(x, want_logits=False)
    with pytest.raises(_lib.LSegError) as e:
        eng.episode_stats(t)
    assert e.value.code == -1 and "5 labels" in str(e.value)
    eng.close()
    # after a labels-only (streamed) forward of a K = 2 label set
    eng, x2 = _tiny512_labels(K=2)
    eng.forward_labels(x2)
    with pytest.raises(_lib.LSegError) as e:
        eng.episode_stats(t)
    assert e.value.code == -4 and "labels-only" in str(e.value)
    eng.forward(x2, want_logits=False)                                             # a shared label set with K = 2 is accepted
    r = eng.episode_stats(t)
    torch.cuda.synchronize()
    assert int(r["areas"][:, 2:4].sum()) == 2 * 64 * 64
    eng.close()


# ---- 5. the whole path --------------------------------------------------------------------------------------------------------------------
def _episode_inputs(B, H, W, seed):
    g = torch.Generator().manual_seed(seed)
    target = torch.randint(0, 2, (B, H, W), generator=g)
    ignore = ((torch.rand(B, H, W, generator=g) < 0.15) & (target == 0)).to(torch.uint8)
    return target, ignore


def _check_whole_path(net, x, ids, nclass):
    B, _, H, W = x.shape
    target, ignore = _episode_inputs(B, H, W, 21)
    with torch.no_grad():
        logits = net(x, ids)
        meter = EpisodeMeter(nclass, range(nclass), "cuda")
        inter, union, loss = net.evaluate_episode(x, ids, target.cuda().float(), ignore=ignore.cuda(), meter=meter)
        i2, u2, l2, lg = net.evaluate_episode(x, torch.tensor(ids), target.cuda(), want_logits=True)
    torch.cuda.synchronize()
    assert torch.equal(lg, logits)
    areas = eh.classify(logits.argmax(1).cpu(), target, ignore)
    ri, ru = eh.inter_union(areas)
    assert inter.dtype == torch.int64 and inter.shape == (2, B) and loss.dim() == 0 and loss.dtype == torch.float32
    assert torch.equal(inter.cpu(), ri) and torch.equal(union.cpu(), ru)
    ri2, ru2 = eh.inter_union(eh.classify(logits.argmax(1).cpu(), target, None))
    assert torch.equal(i2.cpu(), ri2) and torch.equal(u2.cpu(), ru2)
    ref = float(F.cross_entropy(logits.double().view(B, 2, -1), target.cuda().view(B, -1)))
    print(f"{type(net).__name__}: loss {loss.item():.8f} fp64 cross_entropy {ref:.8f} inter {inter.tolist()} union {union.tolist()}")
    assert abs(loss.item() - ref) <= ce_bar(ref) and torch.equal(loss, l2)
    h = eh.Meter(nclass, range(nclass))
    h.update(ri, ru, ids)
    assert torch.equal(meter.intersection_buf.cpu(), h.inter) and torch.equal(meter.union_buf.cpu(), h.union)
    assert len(meter.loss_buf) == 1 and torch.equal(meter.loss_buf[0], loss)
    miou, fb = meter.compute_iou()
    rm, rf = h.compute_iou()
    assert abs(float(miou) - rm) <= 1e-6 * rm and abs(float(fb) - rf) <= 1e-6 * rf


def _zs_module(dataset="fss", **kw):
    warnings.simplefilter("ignore")
    from modules.lseg_module_zs import LSegModuleZS
    m = LSegModuleZS("nowhere", dataset, 2, 0.004, 10, backbone="tiny16", num_features=64, arch_option=0, block_depth=0,
                     activation="lrelu", aux=False, weight_decay=1e-4, use_pretrained="False", **kw)
    m.net.load_state_dict(synthetic_state_dict(get_config("tiny16"), seed=9))
    m.net.cuda()
    return m


def test_evaluate_episode_on_the_tiny_zero_shot_network():
    m = _zs_module()
    m.net.eval()
    _check_whole_path(m.net, synthetic_images(3, 64, 64, seed=9).cuda(), [4, 17, 4], 1000)


def test_evaluate_episode_on_the_resnet101_network():
    from modules.models.lseg_net_zs import LSegRNNetZS
    names = [f"class{i}" for i in range(10)]
    net = LSegRNNetZS(label_list=names, backbone="clip_resnet101", features=256, aux=False, use_pretrained=False, arch_option=0,
                      block_depth=0, activation="lrelu", image_dtype="fp16")
    net.load_state_dict(synthetic_state_dict(get_config("clip_resnet101"), seed=5), strict=False)
    _check_whole_path(net.cuda().eval(), synthetic_images(3, 64, 64, seed=5).cuda(), [3, 7, 7], 10)


# ---- 6. the module ------------------------------------------------------------------------------------------------------------------------
def test_validation_step_and_epoch_end():
    H = W = 64
    m = _zs_module("fss")
    m.dataset = "pascal"                                                           # the 'pascal' rule: the batch's ignore mask is used
    m.net.eval()
    m.val_average_meter = EpisodeMeter("pascal", range(20), "cuda")
    logged = {}
    m.log = lambda k, v, **kw: logged.__setitem__(k, v)
    h = eh.Meter(20, range(20))
    losses = []
    for i, ids in enumerate(([3, 11], [3, 19])):
        target, ignore = _episode_inputs(2, H, W, 30 + i)
        batch = {"query_img": synthetic_images(2, H, W, seed=30 + i).view(2, 1, 3, H, W).cuda(), "query_mask": target.view(2, 1, H, W).float().cuda(),
                 "query_ignore_idx": ignore.view(2, 1, H, W).cuda(), "class_id": torch.tensor(ids).cuda()}
        with torch.no_grad():
            val_loss = m.validation_step(batch, i)
            logits = m.net(batch["query_img"].squeeze(1), ids)
        ri, ru = eh.inter_union(eh.classify(logits.argmax(1).cpu(), target, ignore))
        h.update(ri, ru, ids)
        ref = float(F.cross_entropy(logits.double().view(2, 2, -1), target.cuda().view(2, -1)))
        assert abs(val_loss.item() - ref) <= ce_bar(ref)
        losses.append(ref)
    m.validation_epoch_end([])
    rm, rf = h.compute_iou()
    print(f"logged {[(k, float(v)) for k, v in logged.items()]} helper miou {rm:.6f} fb {rf:.6f}")
    assert set(logged) == {"fewshot_val_loss", "fewshot_val_miou", "fewshot_val_fb_iou"}
    assert abs(float(logged["fewshot_val_miou"]) - rm) <= 1e-6 * rm and abs(float(logged["fewshot_val_fb_iou"]) - rf) <= 1e-6 * rf
    ml = sum(losses) / 2
    assert abs(float(logged["fewshot_val_loss"]) - ml) <= ce_bar(ml)
    # a batch that breaks the reference's assert: ValueError at the epoch end
    target, ignore = _episode_inputs(2, H, W, 40)
    ignore[0, 0, :4] = 1
    target[0, 0, :4] = 1
    batch = {"query_img": synthetic_images(2, H, W, seed=40).view(2, 1, 3, H, W).cuda(), "query_mask": target.view(2, 1, H, W).cuda(),
             "query_ignore_idx": ignore.view(2, 1, H, W).cuda(), "class_id": torch.tensor([0, 1])}
    with torch.no_grad():
        m.validation_step(batch, 2)
    with pytest.raises(ValueError, match="4 pixels"):
        m.validation_epoch_end([])


def test_training_step_with_a_train_average_meter():
    H = W = 64
    m = _zs_module("fss", finetune_mode=True, nshot=1)
    m.net.train()
    g = torch.Generator().manual_seed(11)
    ids = [6, 2]
    batch = {"support_imgs": synthetic_images(2, H, W, seed=12).view(2, 1, 3, H, W).cuda(),
             "support_masks": torch.randint(0, 2, (2, 1, H, W), generator=g).float().cuda(), "class_id": torch.tensor(ids).cuda()}
    img, target, class_info = m.batch_inputs(batch)
    out = m.net(img, class_info).detach()                                          # the train-mode logits (batch-statistics BatchNorm)
    logged = []
    m.log = lambda k, v, **kw: logged.append(k)
    loss0 = m.training_step(batch, 0).detach().clone()
    m.train_average_meter = EpisodeMeter("fss", range(1000), "cuda")
    loss1 = m.training_step(batch, 1)
    torch.cuda.synchronize()
    assert torch.equal(loss0, loss1.detach()), "attaching a meter must not change the step's loss"
    assert logged == ["train_loss", "train_loss"]
    meter = m.train_average_meter
    ri, ru = eh.inter_union(eh.classify(out.argmax(1).cpu(), target.cpu(), None))
    h = eh.Meter(1000, range(1000))
    h.update(ri, ru, ids)
    assert torch.equal(meter.intersection_buf.cpu(), h.inter) and torch.equal(meter.union_buf.cpu(), h.union)
    assert len(meter.loss_buf) == 1 and torch.equal(meter.loss_buf[0], loss1.detach())
    loss1.backward()
