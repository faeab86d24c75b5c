"""Masks for label sets beyond 256 (csrc/corr_argmax.hip, lseg_forward_labels / lseg_op_corr_argmax): the streamed-panel correlation +
arg-max against an fp64 composition (op level), against the engine's own logits and against the reference's 480 x 480 labels (whole
path), plus the int16 fallback and the guards."""
import ctypes as C
import dataclasses
import os
import subprocess
import sys

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

from lseg_hip import _lib                                                        # noqa: E402
from lseg_hip.config import get_config                                           # noqa: E402
from lseg_hip.engine import HipEngine                                            # noqa: E402
from lseg_hip.synth import synthetic_state_dict, fixture_state_dict, synthetic_tokens, synthetic_images   # noqa: E402

_ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    return _lib.load()


def P(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _op_case(B, K, H, W, seed):
    """fp16 g / T with a decisive winner almost everywhere: the base map is made of 3 x 3 blocks, each the text row of one label (x an
    amplitude) + noise, so that margins are O(1) inside a block and cross zero linearly between blocks.  The LAST label duplicates the
    label of block (0, 0): the first of the two must win every pixel either would.  The border of the padded map holds 1e3: a kernel
    that read it would be off by orders of magnitude."""
    gen = torch.Generator().manual_seed(seed)
    T = torch.randn((K, 512), generator=gen)
    T = T / T.norm(dim=-1, keepdim=True)
    hb, wb = (H + 2) // 3, (W + 2) // 3
    lab = torch.randint(0, K - 1, (B, hb, wb), generator=gen)
    T[K - 1] = T[lab[0, 0, 0]]
    T = T.half()
    lab = lab.repeat_interleave(3, 1).repeat_interleave(3, 2)[:, :H, :W]
    amp = 0.75 + 0.5 * torch.rand((B, H, W), generator=gen)
    gi = amp[..., None] * T.float()[lab] + 0.02 * torch.randn((B, H, W, 512), generator=gen)
    g = torch.full((B, H + 2, W + 2, 512), 1000.0)
    g[:, 1:H + 1, 1:W + 1] = gi
    scale = 8.0 + 4.0 * torch.rand((B, 2 * H, 2 * W), generator=gen)
    return g.half().cuda(), T.cuda(), scale.cuda(), int(lab[0, 0, 0])


# (B, K, H, W, seed): the seeds are ones for which the fp64 composition alone leaves <= 0.1 % of the pixels with a top-2 margin under
# 4x the fp16 rounding of the (2h, 2w) logits (the only rounding of the path that is not fp32-small)
OP_CASES = [(1, 16, 6, 6, 1), (2, 157, 15, 15, 2), (1, 158, 30, 30, 3), (2, 300, 9, 17, 4), (1, 1000, 30, 30, 5), (1, 300, 17, 30, 6),
            (1, 1000, 6, 6, 7)]


@pytest.mark.gpu_fast
@pytest.mark.parametrize("B,K,H,W,seed", OP_CASES)
def test_corr_argmax_op_against_fp64(lib, B, K, H, W, seed):
    """lseg_op_corr_argmax vs a plain fp64 torch composition on the same fp16 operands: matmul, x2 bilinear, scale, x2 bilinear, argmax.
    Labels must agree wherever the fp64 top-2 margin exceeds 2x the measured max |score - fp64 value| of the case (the project's "ties"
    criterion); at most 0.1 % of the pixels may be excluded that way.  K = 157 / 158 straddle corr_planes' LDS limit, 300 / 1000 run 7 /
    21 panels with a ragged last one, maps 6 x 6 .. 30 x 30 have one to nine tiles with ragged edges."""
    g, T, scale, dup = _op_case(B, K, H, W, seed)
    guard = 64
    n = B * 16 * H * W
    lbuf = torch.full((n + 2 * guard,), -7, dtype=torch.int16).cuda()
    sbuf = torch.full((n + 2 * guard,), float("nan"), dtype=torch.float32).cuda()
    label = lbuf[guard:guard + n].view(B, 4 * H, 4 * W)
    score = sbuf[guard:guard + n].view(B, 4 * H, 4 * W)
    _lib.check(lib.lseg_op_corr_argmax(P(g), P(T), P(scale), P(label), P(score), B, K, H, W, 512, None, 0, stream()))
    torch.cuda.synchronize()
    assert (lbuf[:guard] == -7).all() and (lbuf[-guard:] == -7).all() and torch.isnan(sbuf[:guard]).all() and torch.isnan(sbuf[-guard:]).all()
    assert torch.isfinite(score).all() and (label >= 0).all() and (label < K).all(), "an output pixel was not written"
    R = torch.einsum("kc,byxc->bkyx", T.double(), g[:, 1:H + 1, 1:W + 1].double())
    mid = F.interpolate(R, scale_factor=2, mode="bilinear", align_corners=True) * scale.double().unsqueeze(1)
    ref = F.interpolate(mid, scale_factor=2, mode="bilinear", align_corners=True)
    # tie rule: the duplicate (last) label never wins; the reference is taken on the set without it
    assert (label == K - 1).sum().item() == 0 and (label == dup).sum().item() > 0
    assert (ref[:, K - 1] - ref[:, dup]).abs().max().item() == 0.0
    ref = ref[:, :K - 1]
    top2 = ref.topk(2, dim=1)
    ref_val, ref_am = top2.values[:, 0], top2.indices[:, 0]
    margin = top2.values[:, 0] - top2.values[:, 1]
    err = (score.double() - ref_val).abs().max().item()
    decisive = margin > 2 * err
    excluded = 1.0 - decisive.double().mean().item()
    print(f"corr_argmax op B={B} K={K} {H}x{W}: max|score - fp64| {err:.3e}, excluded (margin <= 2 err) {excluded:.5f}, "
          f"mismatches at decisive pixels {(label.long()[decisive] != ref_am[decisive]).sum().item()}")
    assert err <= 2e-3 * ref_val.abs().max().item(), err                    # fp16 rounding of the (2h, 2w) logits: 2^-11 relative
    assert excluded <= 1e-3, excluded
    assert torch.equal(label.long()[decisive], ref_am[decisive])
    # without the score output: same labels
    label2 = torch.full_like(label, -7)
    _lib.check(lib.lseg_op_corr_argmax(P(g), P(T), P(scale), P(label2), None, B, K, H, W, 512, None, 0, stream()))
    torch.cuda.synchronize()
    assert torch.equal(label, label2)
    # with a workspace the labels of a tile are split over several workgroups and merged: same labels, same scores, nothing written
    # beyond the outputs
    ws = torch.empty((8 * n * 6 + 4 * guard,), dtype=torch.uint8).cuda()
    lbuf3, sbuf3 = torch.full_like(lbuf, -7), torch.full_like(sbuf, float("nan"))
    _lib.check(lib.lseg_op_corr_argmax(P(g), P(T), P(scale), P(lbuf3[guard:]), P(sbuf3[guard:]), B, K, H, W, 512, P(ws), 8 * n * 6, stream()))
    torch.cuda.synchronize()
    assert torch.equal(lbuf3, lbuf) and torch.equal(sbuf3[guard:guard + n], sbuf[guard:guard + n]) and torch.isnan(sbuf3[:guard]).all() \
        and torch.isnan(sbuf3[-guard:]).all()


def test_corr_argmax_guards(lib):
    g = torch.zeros((1, 6, 6, 512), dtype=torch.float16).cuda()
    T = torch.zeros((40000, 512), dtype=torch.float16).cuda()
    sc = torch.ones((1, 8, 8)).cuda()
    lab = torch.zeros((1, 16, 16), dtype=torch.int16).cuda()
    assert lib.lseg_op_corr_argmax(P(g), P(T), P(sc), P(lab), None, 1, 40000, 4, 4, 512, None, 0, stream()) == -5      # K > 32767: LSEG_ERR_UNSUPPORTED
    assert b"32767" in lib.lseg_last_error(None)
    assert lib.lseg_op_corr_argmax(P(g), P(T), P(sc), P(lab), None, 1, 8, 4, 4, 768, None, 0, stream()) == -5          # other widths
    assert lib.lseg_op_corr_argmax(P(g), P(T), P(sc), None, None, 1, 8, 4, 4, 512, None, 0, stream()) == -1            # NULL label output
    assert lib.lseg_op_corr_argmax(None, P(T), P(sc), P(lab), None, 1, 8, 4, 4, 512, None, 0, stream()) == -1
    assert lib.lseg_op_corr_argmax(P(g), P(T), P(sc), P(lab), None, 1, 8, 1, 4, 512, None, 0, stream()) == -1          # the bilinear needs 2 rows
    assert lib.lseg_op_corr_argmax(P(g), P(T), P(sc), P(lab), None, 600, 8, 1200, 1200, 512, None, 0, stream()) == -5  # beyond 32-bit offsets


# tests/test_gpu_forward.py MASK480_CAPS: (fraction of pixels whose label may differ from the reference's, largest reference margin there)
MASK480_CAPS = {150: {"bf16": (0.035, 0.15), "fp16": (0.005, 0.02), "strict": (0.003, 0.006)},
                1000: {"bf16": (0.14, 0.15), "fp16": (0.026, 0.025), "strict": (0.013, 0.008)}}


@pytest.mark.parametrize("dtype", ["bf16", "fp16", "strict"])
@pytest.mark.parametrize("name", ["ref_full_vitl16_480x480_k1000", "ref_full_vitl16_480x480_k150"])
def test_forward_labels_equals_the_argmax_of_the_engines_own_logits_and_the_reference(name, dtype, golden_dir):
    """forward_labels == forward(x).argmax(1) wherever the engine's own top-2 margin exceeds 1e-6 (<= 0.1 % of the pixels excluded), the
    score equals logits.max(1) BIT FOR BIT there (shared interpolation functions, identical MFMA order), and the labels meet the
    reference's 480 x 480 labels under the caps of the existing mask test.  bf16 / fp16 stream the labels; strict has no commuted
    schedule and takes the int16 fallback.  After a streamed forward the low-resolution logits do not exist: lseg_forward_stats and
    the "lowres" tap refuse."""
    g = torch.load(os.path.join(golden_dir, name + "_out480.pt"))
    bb, H, W, B, K, seed, arch, depth = g["spec"]
    cfg = get_config(bb, arch_option=arch, block_depth=depth, activation="lrelu")
    eng = HipEngine(cfg, H, W, max_batch=B, max_labels=K, image_dtype=dtype)
    eng.load_state_dict(fixture_state_dict(cfg, seed, g))
    eng.set_tokens(g["tokens"])
    x = synthetic_images(B, H, W, seed=seed).cuda()
    lab, score = eng.forward_labels(x, want_score=True)
    torch.cuda.synchronize()
    assert lab.dtype == torch.int16 and lab.shape == (B, H, W) and score.shape == (B, H, W)
    if dtype != "strict":
        with pytest.raises(_lib.LSegError) as e:
            eng.forward_stats(torch.zeros((B, H, W), dtype=torch.long).cuda())
        assert e.value.code == -4 and "labels-only" in str(e.value)                      # LSEG_ERR_STATE
        with pytest.raises(_lib.LSegError) as e:
            eng.intermediate("lowres", (B, K, H // 2, W // 2))
        assert e.value.code == -4 and "labels-only" in str(e.value)
    lab1 = eng.forward_labels(x)                                                         # without the score: same labels
    assert torch.equal(lab, lab1)
    out = eng.forward(x)
    torch.cuda.synchronize()
    top2 = out.topk(2, dim=1)
    decisive = (top2.values[:, 0] - top2.values[:, 1]) > 1e-6
    excluded = 1.0 - decisive.float().mean().item()
    am = top2.indices[:, 0]
    nbad = (lab.long()[decisive] != am[decisive]).sum().item()
    sdiff = (score[decisive] - top2.values[:, 0][decisive]).abs().max().item()
    print(f"{name}[{dtype}]: excluded (own margin <= 1e-6) {excluded:.6f}, label mismatches at decisive pixels {nbad}, "
          f"max|score - logits.max| there {sdiff:.3e}")
    assert excluded <= 1e-3
    assert nbad == 0
    assert torch.equal(score[decisive], top2.values[:, 0][decisive])
    # the tie rule also holds where the margin is 0: the label's own logit equals the maximum everywhere
    assert torch.equal(out.gather(1, lab.long().unsqueeze(1)).squeeze(1), top2.values[:, 0])
    eng.forward_stats(torch.zeros((B, H, W), dtype=torch.long).cuda())                   # planes exist again after a logits forward
    # vs the reference
    ref_am, ref_margin = g["argmax"].long().cuda(), g["margin"].float().cuda()
    mism = lab.long() != ref_am
    frac = mism.float().mean().item()
    worst = ref_margin[mism].max().item() if mism.any() else 0.0
    cap_frac, cap_margin = MASK480_CAPS[K][dtype]
    print(f"{name}[{dtype}] labels vs the reference: mismatch fraction {frac:.5f} (cap {cap_frac}), max reference margin at a mismatch {worst:.4f} (cap {cap_margin})")
    assert frac <= cap_frac and worst <= cap_margin
    if K <= 256:                                              # uint8 stays the default product there, and agrees
        only = eng.forward(x, want_logits=False, want_argmax=True)
        assert only.dtype == torch.uint8 and torch.equal(only.long()[decisive], lab.long()[decisive])
    else:                                                     # the call that used to raise returns the int16 labels
        only = eng.forward(x, want_logits=False, want_argmax=True)
        assert only.dtype == torch.int16 and torch.equal(only, lab)
    eng.close()


@pytest.mark.gpu_fast
@pytest.mark.parametrize("name", ["ref_vitl16_96x96_k5_arch1", "ref_vitl16rn50x16_96x96_k6"])
def test_int16_fallback_equals_the_uint8_masks(name, golden_dir):
    """Head blocks (arch_option 1) and out_c = 768 cannot stream: forward_labels takes the arg-max on the planes in memory, exactly
    where the uint8 masks of lseg_forward are taken, and must equal them; lseg_forward_stats keeps working."""
    g = torch.load(os.path.join(golden_dir, name + ".pt"))
    bb, H, W, B, K, seed, arch, depth = g["spec"]
    cfg = get_config(bb, arch_option=arch, block_depth=depth, activation="lrelu")
    eng = HipEngine(cfg, H, W, max_batch=B, max_labels=K, image_dtype="fp16")
    eng.load_state_dict(synthetic_state_dict(cfg, seed=seed))
    eng.set_tokens(g["tokens"])
    x = synthetic_images(B, H, W, seed=seed).cuda()
    u8 = eng.forward(x, want_logits=False, want_argmax=True)
    lab, score = eng.forward_labels(x, want_score=True)
    r = eng.forward_stats(torch.zeros((B, H, W), dtype=torch.long).cuda())
    assert int(r["labeled"]) == B * H * W
    out = eng.forward(x)
    torch.cuda.synchronize()
    assert u8.dtype == torch.uint8 and lab.dtype == torch.int16
    assert torch.equal(u8.long(), lab.long())
    assert torch.equal(score, out.gather(1, lab.long().unsqueeze(1)).squeeze(1))
    eng.close()


def _tiny512():
    cfg = get_config("tiny16")
    return dataclasses.replace(cfg, out_c=512, text=dataclasses.replace(cfg.text, embed_dim=512))


def _tiny512_labels(K=300):
    cfg = _tiny512()
    eng = HipEngine(cfg, 64, 64, max_batch=2, max_labels=K, image_dtype="fp16")
    eng.load_state_dict(synthetic_state_dict(cfg, seed=3))
    eng.set_tokens(synthetic_tokens([f"thing {i}" for i in range(K)], cfg.text.vocab, cfg.text.ctx))
    return eng, synthetic_images(2, 64, 64, seed=3).cuda()


@pytest.mark.gpu_fast
@pytest.mark.parametrize("wide", [False, True])
def test_per_image_label_sets_take_the_fallback_and_equal_the_uint8_masks(wide):
    """Per-image label sets (lseg_net_zs.py:198-208; 3 images x 2 labels each) cannot stream -- on the tiny network as it is (out_c = 128)
    or widened to out_c = 512, where one shared label set would: the int16 labels are the index within the image's own labels and
    equal the uint8 masks, the score is the label's own logit, and the planes stay in memory.  (The route without the commuted
    schedule is the strict case of the whole-path test above.)"""
    cfg = _tiny512() if wide else get_config("tiny16")
    eng = HipEngine(cfg, 64, 64, max_batch=3, max_labels=6, image_dtype="fp16")
    eng.load_state_dict(synthetic_state_dict(cfg, seed=5))
    eng.set_tokens(synthetic_tokens(["cat", "other", "sky", "other", "tree", "other"], cfg.text.vocab, cfg.text.ctx), labels_per_image=2)
    x = synthetic_images(3, 64, 64, seed=5).cuda()
    u8 = eng.forward(x, want_logits=False, want_argmax=True)
    lab, score = eng.forward_labels(x, want_score=True)
    r = eng.forward_stats(torch.zeros((3, 64, 64), dtype=torch.long).cuda())
    assert int(r["labeled"]) == 3 * 64 * 64
    out = eng.forward(x)
    torch.cuda.synchronize()
    assert out.shape == (3, 2, 64, 64) and lab.dtype == torch.int16 and int(lab.max()) <= 1
    assert torch.equal(u8.long(), lab.long())
    assert torch.equal(score, out.gather(1, lab.long().unsqueeze(1)).squeeze(1))
    eng.close()


_CHILD = """
import sys, torch
sys.path[:0] = [{root!r}, {src!r}, {tests!r}]
import test_gpu_corr_argmax as t
eng, x = t._tiny512_labels()
lab, score = eng.forward_labels(x, want_score=True)
eng.forward_stats(torch.zeros((2, 64, 64), dtype=torch.long).cuda())        # the fallback leaves the planes in memory
torch.cuda.synchronize()
torch.save({{"lab": lab.cpu(), "score": score.cpu()}}, {out!r})
"""


def test_generic_switch_takes_the_fallback_and_agrees_with_the_streamed_labels(tmp_path):
    """A tiny16 network widened to out_c = 512 with K = 300: streamed here, and in a child process under LSEG_CORR_GENERIC=1 (the switch is
    read once per process) through the generic GEMM + planes + int16 fallback.  Equal at the pixels where the engine's own logits are
    decisive.  lseg_forward with a uint8 output still refuses K = 300."""
    eng, x = _tiny512_labels()
    lab, score = eng.forward_labels(x, want_score=True)
    with pytest.raises(_lib.LSegError) as e:
        eng.forward_stats(torch.zeros((2, 64, 64), dtype=torch.long).cuda())
    assert e.value.code == -4                                                  # streamed: LSEG_ERR_STATE
    out = eng.forward(x)
    amax = torch.empty((2, 64, 64), dtype=torch.uint8).cuda()
    rc = eng.lib.lseg_forward(eng._h, P(x), 2, None, P(amax), stream())
    assert rc == -5 and b"uint8" in eng.lib.lseg_last_error(None)              # LSEG_ERR_UNSUPPORTED, as before
    torch.cuda.synchronize()
    top2 = out.topk(2, dim=1).values
    decisive = ((top2[:, 0] - top2[:, 1]) > 1e-6).cpu()
    assert decisive.float().mean().item() >= 0.5            # (the random tiny network ties often; the comparison must not be vacuous)
    path = str(tmp_path / "child.pt")
    env = dict(os.environ, LSEG_CORR_GENERIC="1")
    code = _CHILD.format(root=_ROOT, src=os.path.join(_ROOT, "lang-seg_amd"), tests=os.path.join(_ROOT, "tests"), out=path)
    subprocess.run([sys.executable, "-c", code], env=env, check=True, timeout=600)
    child = torch.load(path)
    assert torch.equal(child["lab"][decisive], lab.cpu()[decisive])
    assert torch.equal(child["score"][decisive], score.cpu()[decisive])
    eng.close()


def test_predict_labels_of_the_network_module():
    """LSegNet.predict_labels = torch.max(net(x, labelset), 1)[1] as torch.long, for a label set beyond 256."""
    from modules.models.lseg_net import LSegNet
    labels = [f"thing {i}" for i in range(300)]
    cfg = get_config("tiny16")
    net = LSegNet(labels=labels, backbone="tiny16", features=cfg.features, arch_option=0, block_depth=0, activation="lrelu")
    net.load_state_dict(synthetic_state_dict(cfg, seed=0))
    net = net.eval().cuda()
    x = synthetic_images(2, 64, 64, seed=0).cuda()
    with torch.no_grad():
        out = net(x)
    lab = net.predict_labels(x)
    assert lab.dtype == torch.long and lab.shape == (2, 64, 64)
    top2 = out.topk(2, dim=1)
    decisive = (top2.values[:, 0] - top2.values[:, 1]) > 1e-6
    assert torch.equal(lab[decisive], top2.indices[:, 0][decisive])
