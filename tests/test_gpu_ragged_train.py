"""The ragged training step (lseg_set_text_groups in train mode) on the GPU: image b is scored against its own k_b labels, the loss is
sum(nll) / sum(valid pixels) over the batch, one train-mode forward of the image tower.

  1. the two kernels of csrc/ragged_train.hip against float64 autograd (tests/ragged_train_helpers.py), with the error bar MEASURED on
     the shared-set kernels they restate (seg_stats + upsample_ce_backward_rows at uniform K = 9 and K = 70 on tensors of the same
     kind): the ragged kernels do the same arithmetic and get 2x that error; columns >= k_b of the rows are exactly zero;
  2. the whole step on tiny16 against the oracle composed per image (train-mode tower once, each image against its own text rows);
  3. B equal lists against the shared-set step with that list: bit-equal planes, equal loss, close gradients;
  4. isolation: replacing image 2's labels leaves image 0's planes and log-sum-exp bit-identical;
  5. the refusals.

  6. the correlation (lseg_op_corr_ragged_fwd / _bwd) in both stages -- 1: the generic GEMM per image, 2: one launch for the batch -- at
     C in {128, 512, 768}: stage-two planes bit-equal to stage one, both against a float64 product within fp16 half-ulp + the fp32
     accumulation bound; backward of each stage against float64 with the shared chain (GEMM + l2norm_scale_backward at uniform K = 9
     and K = 70) as the yardstick, 2x its error;
  7. the Python surface: LSegNet.forward_loss with a list of lists and DataParallelTrainer.forward_backward equal the engine step.

The engine tests run on stage two (the default); the equal-lists test therefore also holds stage two's planes against the shared set's.
"""
import math
import ctypes as C

import pytest
import torch

pytestmark = pytest.mark.gpu

from lseg_hip import _lib                                                         # noqa: E402
from lseg_hip.config import get_config                                            # noqa: E402
from lseg_hip.engine import HipEngine                                             # noqa: E402
from lseg_hip.synth import synthetic_state_dict, synthetic_tokens, synthetic_images   # noqa: E402
from ragged_train_helpers import (make_planes, make_targets, oracle_ragged_step, prefix_of,   # noqa: E402
                                  ragged_rows_reference)
from train_helpers import cosine, rel                                             # noqa: E402

COUNTS = [1, 9, 70]            # 1: the degenerate softmax; 9: the first count the grouped kernel cannot take; 70: crosses the 64-column pad
H_LOW, W_LOW = 24, 20          # not square; 480 low-resolution pixels per image are a multiple of neither 256 nor 64
IGN = -100
WORDS = [f"thing{i} kind{i % 7}" for i in range(80)]


def P(t):
    return C.c_void_p(t.data_ptr())


def _st():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _up64(v):
    return (v + 63) // 64 * 64


# ---- 1. the kernels ------------------------------------------------------------------------------------------------------------------
def _run_ragged_ops(planes, target, counts, ldk, gscale=None):
    lib = _lib.load()
    B, (h, w) = len(counts), planes[0].shape[1:]
    low = torch.cat([p.reshape(-1) for p in planes]).cuda()
    t = target.cuda()
    cnt = (C.c_int32 * B)(*counts)
    prefix = torch.zeros(B + 1, dtype=torch.int32, device="cuda")
    nll = torch.zeros(2, dtype=torch.float64, device="cuda")
    c2 = torch.zeros(2, dtype=torch.int64, device="cuda")
    lse = torch.full((B, 2 * h, 2 * w), float("nan"), device="cuda")
    _lib.check(lib.lseg_op_ragged_ce_fwd(P(low), P(t), cnt, P(prefix), B, h, w, IGN, P(nll), P(c2), P(lse), _st()))
    torch.cuda.synchronize()
    fwd = (nll.cpu().clone(), c2.cpu().clone(), lse.cpu().clone(), prefix.cpu().clone())
    rows = torch.full((B * h * w, ldk), float("nan"), dtype=torch.float16, device="cuda")
    lse2 = torch.empty_like(lse)
    gs = torch.tensor([gscale], dtype=torch.float32, device="cuda") if gscale is not None else None
    _lib.check(lib.lseg_op_ragged_ce_bwd_rows(P(low), P(t), cnt, P(prefix), B, h, w, IGN, P(nll), P(lse2), P(rows), ldk, _lib.LSEG_F16,
                                              P(gs) if gs is not None else None, _st()))
    torch.cuda.synchronize()
    assert torch.equal(lse2.cpu(), fwd[2])
    return fwd, rows.cpu()


def _run_shared_ops(planes, target, K, ldk):
    """the shared-set kernels the ragged ones restate, on a rectangular batch: seg_stats (through the bilinear) + upsample_ce_backward_rows"""
    lib = _lib.load()
    B, (h, w) = len(planes), planes[0].shape[1:]
    low = torch.stack(planes).cuda()
    t = target.cuda()
    nll = torch.zeros(2, dtype=torch.float64, device="cuda")
    lse = torch.empty((B, 2 * h, 2 * w), device="cuda")
    rows = torch.full((B * h * w, ldk), float("nan"), dtype=torch.float16, device="cuda")
    _lib.check(lib.lseg_op_upsample_ce_backward_rows(P(low), P(t), B, K, h, w, IGN, P(nll), P(lse), P(rows), ldk, _lib.LSEG_F16, _st()))
    torch.cuda.synchronize()
    return nll.cpu(), lse.cpu(), rows.cpu()


def _errors(nll, lse, rows, ref):
    _, ref_nll, valid, ref_lse, ref_rows = ref
    assert int(nll[1]) == valid
    return {"nll_rel": abs(float(nll[0]) - ref_nll) / abs(ref_nll),
            "lse_maxabs": (lse.double() - torch.stack(ref_lse)).abs().max().item(),
            "rows_maxabs": (rows.double() - ref_rows).abs().max().item(),
            "rows_1mcos": 1.0 - cosine(rows, ref_rows)}


@pytest.mark.parametrize("ignored_image", [None, 0])
def test_ragged_loss_kernels_against_float64_within_twice_the_shared_kernels_error(ignored_image):
    h, w, B = H_LOW, W_LOW, len(COUNTS)
    ldk = _up64(max(COUNTS))
    target = make_targets(COUNTS, 2 * h, 2 * w, seed=11, ignored_image=ignored_image)
    planes = make_planes(COUNTS, h, w, seed=12)
    (nll, c2, lse, prefix), rows = _run_ragged_ops(planes, target, COUNTS, ldk)
    assert prefix.tolist() == prefix_of(COUNTS)
    ref = ragged_rows_reference(planes, target, ldk, IGN)
    err = _errors(nll, lse, rows, ref)
    # the yardstick: the shared-set kernels against float64 on rectangular batches of the same kind of planes, the same ignore mask
    # (hence the same number of valid pixels and the same 1 / n scale of the rows), at the two counts that are not degenerate
    base = {}
    for K in (9, 70):
        tK = make_targets([K] * B, 2 * h, 2 * w, seed=11, ignored_image=ignored_image)
        pK = make_planes([K] * B, h, w, seed=12 + K)
        e = _errors(*_run_shared_ops(pK, tK, K, ldk), ragged_rows_reference(pK, tK, ldk, IGN))
        print(f"shared-set kernels K={K} ignored_image={ignored_image}: " + ", ".join(f"{k} {v:.3e}" for k, v in e.items()))
        base = {k: max(v, base.get(k, 0.0)) for k, v in e.items()}
    print(f"ragged kernels counts={COUNTS} ignored_image={ignored_image}: " + ", ".join(f"{k} {v:.3e}" for k, v in err.items()))
    for k in err:
        assert err[k] <= 2.0 * base[k], (k, err[k], base[k])
    # dev_grad_scale (what loss.backward() hands down through lseg_backward_scaled): the rows are the scaled gradient
    _, rows_s = _run_ragged_ops(planes, target, COUNTS, ldk, gscale=0.37)
    gs = float(torch.tensor(0.37, dtype=torch.float32))
    es = (rows_s.double() - gs * ref[4]).abs().max().item()
    print(f"ragged rows with grad scale 0.37: rows_maxabs {es:.3e}")
    assert es <= 2.0 * base["rows_maxabs"] and not torch.equal(rows_s, rows)
    # columns >= k_b: exactly zero, written (the buffer was NaN)
    for b, kb in enumerate(COUNTS):
        blk = rows[b * h * w:(b + 1) * h * w]
        assert (blk[:, kb:] == 0).all() and torch.isfinite(blk).all()
    assert (rows[:h * w] == 0).all()                                     # one label: softmax - onehot = 0 (and an ignored image: no gradient)
    # {correct, labeled}: labeled counts every target >= 0 (seg_stats' rule); correct against the float64 arg-max, up to near-ties
    from ragged_train_helpers import upsample2x_f64
    pred = torch.stack([upsample2x_f64(p.double()).argmax(0) for p in planes])
    assert int(c2[1]) == int((target >= 0).sum())
    assert abs(int(c2[0]) - int((pred == target).sum())) <= 2


def test_ragged_ops_refuse_bad_arguments():
    lib = _lib.load()
    z = torch.zeros(4096, device="cuda")
    t = torch.zeros((1, 8, 8), dtype=torch.int64, device="cuda")
    d = torch.zeros(2, dtype=torch.float64, device="cuda")
    i2 = torch.zeros(2, dtype=torch.int64, device="cuda")
    pre = torch.zeros(2, dtype=torch.int32, device="cuda")
    assert lib.lseg_op_ragged_ce_fwd(P(z), P(t), (C.c_int32 * 1)(0), P(pre), 1, 4, 4, IGN, P(d), P(i2), P(z), _st()) == -1      # a count of 0
    assert lib.lseg_op_ragged_ce_bwd_rows(P(z), P(t), (C.c_int32 * 1)(9), P(pre), 1, 4, 4, IGN, P(d), P(z), P(z), 8, _lib.LSEG_F16, None,
                                          _st()) == -1                                                                       # ldk < count
    assert lib.lseg_op_ragged_ce_bwd_rows(P(z), P(t), (C.c_int32 * 1)(2), P(pre), 1, 4, 4, IGN, P(d), P(z), P(z), 12, _lib.LSEG_F16, None,
                                          _st()) == -1                                                                       # ldk % 8


# ---- engine-level helpers --------------------------------------------------------------------------------------------------------------
def _tokens(cfg, lists):
    return synthetic_tokens([w for ls in lists for w in ls], cfg.text.vocab, cfg.text.ctx)


def _lists(counts, start=0):
    out, i = [], start
    for k in counts:
        out.append(WORDS[i:i + k])
        i += k
    return out


def _ragged_step(cfg, sd, x, target, lists, want_planes=False):
    B, _, H, W = x.shape
    counts = [len(ls) for ls in lists]
    tok = _tokens(cfg, lists)
    sd_dev = {k: v.clone().cuda() for k, v in sd.items()}
    eng = HipEngine(cfg, H, W, max_batch=B, max_labels=tok.shape[0])
    eng.load_state_dict(sd_dev)
    eng.set_tokens(tok, group_sizes=counts)
    eng.enable_training(sd_dev)
    assert eng.forward(x.cuda(), want_logits=False) is None
    planes = eng.intermediate("lowres", (sum(counts), H // 2, W // 2)).cpu() if want_planes else None
    loss = eng.backward(target=target.cuda(), ignore_index=IGN)
    torch.cuda.synchronize()
    return eng, loss, planes


def _tiny():
    cfg = get_config("tiny16")
    return cfg, synthetic_state_dict(cfg, seed=21), synthetic_images(3, 64, 64, seed=21)


# ---- 2. whole step against the oracle --------------------------------------------------------------------------------------------------
def test_ragged_training_step_matches_the_per_image_oracle():
    cfg, sd, x = _tiny()
    lists = _lists(COUNTS)
    target = make_targets(COUNTS, 64, 64, seed=22)
    ref_loss, ref_grads = oracle_ragged_step(sd, x, target, _tokens(cfg, lists), COUNTS, cfg, IGN)
    eng, loss, _ = _ragged_step(cfg, sd, x, target, lists)
    assert abs(loss.item() - ref_loss) <= 1e-2 * abs(ref_loss), (loss.item(), ref_loss)
    assert set(eng.grads) == set(ref_grads), sorted(set(eng.grads) ^ set(ref_grads))[:10]
    report = {k: rel(eng.grads[k].cpu(), ref_grads[k]) for k in ref_grads}
    nerr = {k: abs(eng.grads[k].norm().item() - ref_grads[k].norm().item()) / ref_grads[k].norm().item() for k in ref_grads}
    print(f"ragged step {COUNTS}: loss {loss.item():.5f} vs {ref_loss:.5f}; median / max gradient error "
          f"{sorted(report.values())[len(report) // 2]:.4f} / {max(report.values()):.4f}; max norm error {max(nerr.values()):.4f}")
    # the bars of the uniform per-image training test (test_gpu_train_zs.test_zero_shot_training_step_matches_the_oracle)
    assert max(report.values()) <= 0.35 and max(nerr.values()) <= 0.15
    # train_loss: the same value without the backward, and the batch's {correct, labeled}
    eng.forward(x.cuda(), want_logits=False)
    l2, cnt = eng.train_loss(target.cuda(), IGN, want_counts=True)
    assert abs(l2.item() - loss.item()) <= 1e-6 * abs(loss.item())
    assert int(cnt[1]) == int((target >= 0).sum()) and 0 <= int(cnt[0]) <= int(cnt[1])
    eng.close()


# ---- 3. equal lists = the shared-set step ----------------------------------------------------------------------------------------------
def test_equal_lists_equal_the_shared_set_step():
    cfg, sd, x = _tiny()
    B, K = 3, 9
    one = WORDS[:K]
    target = make_targets([K] * B, 64, 64, seed=23)
    er, lr_, pr = _ragged_step(cfg, sd, x, target, [one] * B, want_planes=True)
    nll_r = er._loss.cpu().clone()
    sd_dev = {k: v.clone().cuda() for k, v in sd.items()}
    es = HipEngine(cfg, 64, 64, max_batch=B, max_labels=K)
    es.load_state_dict(sd_dev)
    es.set_tokens(synthetic_tokens(one, cfg.text.vocab, cfg.text.ctx))
    es.enable_training(sd_dev)
    es.forward(x.cuda(), want_logits=False)
    ps = es.intermediate("lowres", (B, K, 32, 32)).cpu()
    es.backward(target=target.cuda(), ignore_index=IGN)
    torch.cuda.synchronize()
    nll_s = es._loss.cpu().clone()
    assert torch.equal(pr.view(B, K, 32, 32), ps)                                       # the planes, bit for bit
    assert nll_r[1] == nll_s[1]
    assert abs(float(nll_r[0]) - float(nll_s[0])) <= 1e-12 * abs(float(nll_s[0])), (nll_r, nll_s)     # double sums in another order
    r = {k: rel(er.grads[k], es.grads[k]) for k in es.grads}
    print(f"equal lists vs shared set: gradients median rel diff {sorted(r.values())[len(r) // 2]:.2e}, worst {max(r.values()):.2e}")
    assert set(er.grads) == set(es.grads) and max(r.values()) <= 0.35
    er.close(); es.close()


# ---- 4. isolation -----------------------------------------------------------------------------------------------------------------------
def test_another_images_labels_do_not_touch_image_zero():
    """The planes are read from the engine ("lowres" tap).  The engine's own per-pixel log-sum-exp buffer has no tap and is NOT read here:
    the log-sum-exp compared below is the loss kernel's output on those planes (the same launcher the engine calls)."""
    cfg, sd, x = _tiny()
    target = make_targets(COUNTS, 64, 64, seed=24)
    la = _lists(COUNTS)
    lb = [la[0], la[1], WORDS[5:75][::-1]]                                              # image 2: other labels, same count
    ea, _, pa = _ragged_step(cfg, sd, x, target, la, want_planes=True)
    eb, _, pb = _ragged_step(cfg, sd, x, target, lb, want_planes=True)
    n0 = COUNTS[0]
    assert torch.equal(pa[:n0 + COUNTS[1]], pb[:n0 + COUNTS[1]])                        # images 0 and 1: bit-identical planes
    assert not torch.equal(pa[n0 + COUNTS[1]:], pb[n0 + COUNTS[1]:])
    lses = []
    for p in (pa, pb):                                                                   # the per-pixel log-sum-exp the loss kernel leaves
        planes = [p[a:b] for a, b in zip(prefix_of(COUNTS)[:-1], prefix_of(COUNTS)[1:])]
        (_, _, lse, _), _ = _run_ragged_ops(planes, target, COUNTS, 128)
        lses.append(lse)
    assert torch.equal(lses[0][0], lses[1][0]) and not torch.equal(lses[0][2], lses[1][2])
    ea.close(); eb.close()


# ---- 5. refusals -----------------------------------------------------------------------------------------------------------------------
def test_ragged_training_refusals():
    cfg, sd, x = _tiny()
    lib = _lib.load()
    lists = _lists([2, 3, 4])
    counts = [2, 3, 4]
    tok = _tokens(cfg, lists)
    sd_dev = {k: v.cuda() for k, v in sd.items()}
    eng = HipEngine(cfg, 64, 64, max_batch=3, max_labels=9)
    eng.load_state_dict(sd_dev)
    eng.set_tokens(tok, group_sizes=counts)
    eng.enable_training(sd_dev)
    xd = x.cuda()
    with pytest.raises(_lib.LSegError, match="logits"):                                 # logits output requested
        eng.forward(xd)
    out = torch.empty((3, 9, 64, 64), device="cuda")
    assert lib.lseg_forward(eng._h, P(xd), 3, P(out), None, _st()) == -5
    eng.forward(xd, want_logits=False)
    with pytest.raises(_lib.LSegError, match="target"):                                 # d(logits) hand-over
        eng.backward(dlogits=out)
    assert lib.lseg_forward(eng._h, P(xd), 2, None, None, _st()) == -1                  # number of lists != B
    with pytest.raises(ValueError, match="label lists != batch"):
        eng.forward(xd[:2], want_logits=False)
    with pytest.raises(ValueError, match=">= 1 label"):                                 # a count of 0
        eng.set_tokens(tok, group_sizes=[5, 0, 4])
    assert lib.lseg_set_text_groups(eng._h, (C.c_int32 * 3)(5, 0, 4), 3) == -1
    with pytest.raises(ValueError, match="max_labels"):                                 # a count above max_labels
        eng.set_tokens(tok, group_sizes=[10])
    assert lib.lseg_set_text_groups(eng._h, (C.c_int32 * 1)(10), 1) == -1
    with pytest.raises(ValueError, match="int64"):                                      # the target's dtype
        eng.set_tokens(tok, group_sizes=counts)
        eng.forward(xd, want_logits=False)
        eng.backward(target=torch.zeros((3, 64, 64), dtype=torch.int32, device="cuda"))
    eng.close()
    cfg1 = get_config("tiny16", arch_option=1, block_depth=1)                           # arch_option 1
    sd1 = {k: v.cuda() for k, v in synthetic_state_dict(cfg1, seed=1).items()}
    e1 = HipEngine(cfg1, 64, 64, max_batch=3, max_labels=9, head_block_training=True)
    e1.load_state_dict(sd1)
    e1.set_tokens(tok, group_sizes=counts)
    with pytest.raises(_lib.LSegError, match="arch_option"):
        e1.set_train(True)
    e1.close()


# ---- 6. the per-image correlation at the widths the networks use -----------------------------------------------------------------------
SCALE = math.exp(math.log(1 / 0.07))
HW = H_LOW * W_LOW


def _f16_ulp(v):
    e = torch.floor(torch.log2(v.double().abs().clamp_min(2.0 ** -14)))
    return torch.pow(2.0, e - 10)


def _corr_inputs(Cc, counts, seed):
    g = torch.Generator().manual_seed(seed)
    B = len(counts)
    f = torch.randn(B * HW, Cc, generator=g) + 0.3
    a16 = (SCALE * (f / f.norm(dim=-1, keepdim=True)).half().float()).half()
    t = torch.randn(sum(counts), Cc, generator=g)
    t16 = (t / t.norm(dim=-1, keepdim=True)).half()
    return f, a16, t16


@pytest.mark.parametrize("Cc", [128, 512, 768])
def test_ragged_correlation_forward_against_float64(Cc):
    lib = _lib.load()
    B, pre = len(COUNTS), prefix_of(COUNTS)
    _, a16, t16 = _corr_inputs(Cc, COUNTS, seed=31 + Cc)
    a_d, t_d = a16.cuda(), t16.cuda()
    planes = {}
    for stage in (1, 2):
        low = torch.full((sum(COUNTS) * HW,), float("nan"), device="cuda")
        _lib.check(lib.lseg_op_corr_ragged_fwd(P(a_d), P(t_d), P(low), (C.c_int32 * B)(*COUNTS), B, HW, Cc, stage, _st()))
        torch.cuda.synchronize()
        planes[stage] = low.cpu()
    same = (planes[1] == planes[2]).float().mean().item()
    print(f"ragged correlation forward C={Cc}: stage two == stage one on {same:.6f} of the logits, max diff "
          f"{(planes[1] - planes[2]).abs().max().item():.3g}")
    assert torch.equal(planes[1], planes[2])                                             # the one-launch kernel: bit-equal to the per-image GEMM
    got = planes[2].double()
    assert torch.equal(got, got.half().double())                                         # fp16 values, every plane written
    worst = 0.0
    for b in range(B):
        A, T = a16[b * HW:(b + 1) * HW].double(), t16[pre[b]:pre[b + 1]].double()
        ref = (A @ T.t()).t()                                                            # [k_b, hw]
        # fp32 accumulation of C exact fp16 x fp16 products, in any order: |acc - exact| <= C * 2^-24 * sum |a_i t_i|; then ONE rounding
        # to fp16: half an fp16 ulp at the accumulated value (taken at |ref| + the accumulation bound, so a binade edge cannot bite)
        acc = Cc * 2.0 ** -24 * (A.abs() @ T.abs().t()).t()
        bound = acc + 0.5 * _f16_ulp(ref.abs() + acc)
        d = (got[pre[b] * HW:pre[b + 1] * HW].view(-1, HW) - ref).abs()
        worst = max(worst, (d / bound).max().item())
        assert (d <= bound).all(), (b, (d / bound).max().item())
    print(f"ragged correlation forward C={Cc}: worst error / bound {worst:.3f}")


def _corr_bwd_reference(rows, t16, feat, counts, bf16_mode):
    """fp64: dA_b = rt(rows_b[:, :k_b] . T_b) -> fp16(scale dA) (fp16 rows) | dA (bf16 rows, scale applied after) -> L2-norm backward"""
    dt = torch.bfloat16 if bf16_mode else torch.float16
    T = t16.to(dt).double() if bf16_mode else t16.double()
    pre = prefix_of(counts)
    dA = torch.cat([rows[b * HW:(b + 1) * HW, :k].double() @ T[pre[b]:pre[b + 1]] for b, k in enumerate(counts)]).to(dt).double()
    gvec = dA if bf16_mode else (SCALE * dA).half().double()
    post = SCALE if bf16_mode else 1.0
    xd = feat.double()
    n2 = (xd * xd).sum(-1, keepdim=True)
    return post * (gvec - xd * (xd * gvec).sum(-1, keepdim=True) / n2) / n2.sqrt()


def _rows_for(counts, ldk, dt, seed):
    g = torch.Generator().manual_seed(seed)
    rows = torch.zeros(len(counts) * HW, ldk)
    for b, k in enumerate(counts):
        rows[b * HW:(b + 1) * HW, :k] = torch.randn(HW, k, generator=g) * 1e-3
    return rows.to(dt)


@pytest.mark.parametrize("stage", [1, 2])
@pytest.mark.parametrize("Cc,mode", [(128, "fp16_rows"), (512, "fp16_rows"), (768, "fp16_rows"), (512, "bf16_rows")])
def test_ragged_correlation_backward_against_float64_within_twice_the_shared_chain(Cc, mode, stage):
    lib = _lib.load()
    bf = mode == "bf16_rows"
    dt, rdt = (torch.bfloat16, _lib.LSEG_BF16) if bf else (torch.float16, _lib.LSEG_F16)
    B, ldk = len(COUNTS), _up64(max(COUNTS))

    def errors(got, ref):
        return {"maxabs": (got.double() - ref).abs().max().item(), "1mcos": 1.0 - cosine(got, ref)}

    # the yardstick: the shared chain (one label set for the batch) GEMM(rows x T^T) + l2norm_scale_backward against float64
    base = {}
    for K in (9, 70):
        f, _, t16 = _corr_inputs(Cc, [K], seed=41 + K)
        f = torch.randn(B * HW, Cc, generator=torch.Generator().manual_seed(43 + K)) + 0.3
        Kp = _up64(K)
        rows = _rows_for([K] * B, Kp, dt, seed=45 + K)
        tT = torch.zeros(Cc, Kp, dtype=dt)
        tT[:, :K] = t16.to(dt).t()
        r_d, t_d, f_d = rows.cuda(), tT.cuda(), f.cuda()
        zb = torch.zeros(Cc, device="cuda")
        da = torch.empty(B * HW, Cc, dtype=dt, device="cuda")
        df = torch.empty(B * HW, Cc, dtype=torch.bfloat16, device="cuda")
        _lib.check(lib.lseg_op_gemm(P(r_d), P(t_d), P(zb), None, P(da), B * HW, Cc, Kp, rdt, rdt, 0, _st()))
        _lib.check(lib.lseg_op_l2norm_scale_backward(P(da), rdt, P(f_d), P(df), _lib.LSEG_BF16, B * HW, Cc, C.c_float(SCALE), _st()))
        torch.cuda.synchronize()
        ref = _corr_bwd_reference(rows, torch.cat([t16] * B), f, [K] * B, bf)
        e = errors(df.cpu(), ref)
        print(f"shared chain K={K} C={Cc} {mode}: " + ", ".join(f"{k} {v:.3e}" for k, v in e.items()))
        base = {k: max(v, base.get(k, 0.0)) for k, v in e.items()}
    f, _, t16 = _corr_inputs(Cc, COUNTS, seed=47)
    rows = _rows_for(COUNTS, ldk, dt, seed=48)
    r_d, t_d, f_d = rows.cuda(), t16.cuda(), f.cuda()
    df = torch.full((B * HW, Cc), float("nan"), dtype=torch.bfloat16, device="cuda")
    _lib.check(lib.lseg_op_corr_ragged_bwd(P(r_d), rdt, ldk, P(t_d), P(f_d), P(df), _lib.LSEG_BF16, (C.c_int32 * B)(*COUNTS), B, HW, Cc,
                                           C.c_float(SCALE), stage, _st()))
    torch.cuda.synchronize()
    ref = _corr_bwd_reference(rows, t16, f, COUNTS, bf)
    got = df.cpu()
    assert torch.isfinite(got).all()
    err = errors(got, ref)
    print(f"ragged correlation backward stage {stage} counts={COUNTS} C={Cc} {mode}: " + ", ".join(f"{k} {v:.3e}" for k, v in err.items()))
    for k in err:
        assert err[k] <= 2.0 * base[k], (k, err[k], base[k])
    # per image as well: a wrong panel offset or pitch on the small images would hide in the batch maximum
    for b in range(B):
        sl = slice(b * HW, (b + 1) * HW)
        eb = errors(got[sl], ref[sl])
        assert eb["maxabs"] <= 2.0 * base["maxabs"] and eb["1mcos"] <= 2.0 * base["1mcos"], (b, eb, base)


def test_ragged_correlation_ops_refuse_bad_arguments():
    lib = _lib.load()
    z = torch.zeros(64 * 128, dtype=torch.float16, device="cuda")
    f = torch.zeros(64 * 128, device="cuda")
    out = (C.c_int * 8)()
    assert lib.lseg_op_corr_ragged_plan((C.c_int32 * 2)(8, 9), 2, 480, 512, out) == 0 and list(out) == [2, 3, 128, 64, 17, 2 * 480 * 512, 16, 60]
    assert lib.lseg_op_corr_ragged_plan((C.c_int32 * 1)(3), 1, 4, 96, out) == -5                       # C % 64
    assert lib.lseg_op_corr_ragged_fwd(P(z), P(z), P(f), (C.c_int32 * 1)(0), 1, 4, 128, 2, _st()) == -1   # a count of 0
    assert lib.lseg_op_corr_ragged_fwd(P(z), P(z), P(f), (C.c_int32 * 1)(2), 1, 4, 128, 3, _st()) == -1   # no such stage
    assert lib.lseg_op_corr_ragged_bwd(P(z), _lib.LSEG_F16, 64, P(z), P(f), P(z), _lib.LSEG_BF16, (C.c_int32 * 1)(70), 1, 4, 128,
                                       C.c_float(1.0), 2, _st()) == -1                              # ldk < up64(count)


# ---- 7. the Python surface --------------------------------------------------------------------------------------------------------------
def test_forward_loss_with_label_lists_and_the_trainer_equal_the_engine_step():
    from lseg_hip.train import DataParallelTrainer
    from modules.models.lseg_net import LSegNet, tokenize
    cfg, sd, x = _tiny()
    counts = [2, 3, 4]
    lists = _lists(counts)
    target = make_targets(counts, 64, 64, seed=25)
    tok = tokenize([w for ls in lists for w in ls], cfg.text.ctx, cfg.text.vocab)     # image 0's labels first, as forward_loss flattens them
    # the engine step on those token rows
    sd_dev = {k: v.clone().cuda() for k, v in sd.items()}
    eng = HipEngine(cfg, 64, 64, max_batch=3, max_labels=tok.shape[0])
    eng.load_state_dict(sd_dev)
    eng.set_tokens(tok, group_sizes=counts)
    eng.enable_training(sd_dev)
    eng.forward(x.cuda(), want_logits=False)
    loss_e = eng.backward(target=target.cuda(), ignore_index=IGN)
    torch.cuda.synchronize()
    ge = {k: v.clone() for k, v in eng.grads.items()}
    eng.close()
    # DataParallelTrainer (one process): forward_backward passes through HipEngine with the groups set
    sd_dev2 = {k: v.clone().cuda() for k, v in sd.items()}
    e2 = HipEngine(cfg, 64, 64, max_batch=3, max_labels=tok.shape[0])
    e2.load_state_dict(sd_dev2)
    e2.set_tokens(tok, group_sizes=counts)
    tr = DataParallelTrainer(e2, sd_dev2, sync_bn=False)
    loss_t = tr.forward_backward(x.cuda(), target.cuda(), ignore_index=IGN)
    torch.cuda.synchronize()
    assert loss_t.item() == loss_e.item() and not [k for k in ge if not torch.equal(ge[k], e2.grads[k])]
    e2.close()
    # LSegNet.forward_loss(x, target, list of lists) under autograd
    net = LSegNet(labels=["a", "b"], backbone="tiny16", features=cfg.features, arch_option=0, block_depth=0, activation="lrelu")
    net.load_state_dict(sd)
    net = net.cuda().train()
    loss_n = net.forward_loss(x.cuda(), target.cuda(), lists, ignore_index=IGN)
    loss_n.backward()
    torch.cuda.synchronize()
    assert abs(loss_n.item() - loss_e.item()) <= 1e-6 * abs(loss_e.item()), (loss_n.item(), loss_e.item())
    named = dict(net.named_parameters())
    r = {k: rel(named[k].grad, ge[k]) for k in ge}
    print(f"forward_loss(list of lists) vs engine step: loss {loss_n.item():.6f} / {loss_e.item():.6f}, worst gradient rel diff {max(r.values()):.2e}")
    assert max(r.values()) <= 1e-5
    assert net._last_train_counts is not None and int(net._last_train_counts[1]) == int((target >= 0).sum())
    # a second call with other lists of the same sizes must not reuse the cached tokens
    l2 = net.forward_loss(x.cuda(), target.cuda(), [lists[0], lists[1], WORDS[40:44]], ignore_index=IGN)
    assert abs(l2.item() - loss_n.item()) > 1e-6 * abs(loss_n.item())
