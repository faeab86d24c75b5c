"""Decoded uint8 HWC images in (lseg_set_input_u8, csrc/input_u8.hip): every result must be the SAME BITS as the float path fed the
tensor ToTensor + Normalize make of the image -- op level (patch rows, ResNet stem, evaluator crops), whole forwards of the three
network kinds, the training step, the multi-scale evaluator -- and every refusal returns its documented status.  The float reference
inputs are built on the host (input_u8_helpers.to_tensor_normalize says why)."""
import ctypes as C
import math

import pytest
import torch

from lseg_hip import _lib
from lseg_hip.config import get_config
from lseg_hip.engine import HipEngine
from lseg_hip.evaluator import BatchedMultiEval, ModuleSurface, scale_geometry
from lseg_hip.synth import synthetic_state_dict, synthetic_tokens

from input_u8_helpers import HALF, IMAGENET, images_u8, to_tensor_normalize

pytestmark = pytest.mark.gpu

DT = {"bf16": (torch.bfloat16, _lib.LSEG_BF16), "fp16": (torch.float16, _lib.LSEG_F16)}
SENTINEL = 0x7B7B                     # guard-band word: a finite 16-bit pattern no kernel here writes in bulk
GUARD = 256                           # guard elements on each side of an output


@pytest.fixture(scope="module")
def lib():
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    return _lib.load()


def P(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def F3(v):
    return (C.c_float * 3)(*[float(a) for a in v])


def guarded(n):
    """int16 device buffer of GUARD + n + GUARD sentinel words and the view of its middle (16-byte aligned: GUARD * 2 bytes)"""
    buf = torch.full((GUARD + n + GUARD,), SENTINEL, dtype=torch.int16, device="cuda")
    return buf, buf[GUARD:GUARD + n]


def guards_untouched(buf, n):
    return bool((buf[:GUARD] == SENTINEL).all()) and bool((buf[GUARD + n:] == SENTINEL).all())


# ---- 1. op level: the patch-embedding operand rows ----------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["bf16", "fp16"])
@pytest.mark.parametrize("kind", ["arange", "random"])
@pytest.mark.parametrize("B,H,W,patch", [(1, 32, 48, 16), (3, 32, 48, 16), (1, 64, 64, 16), (3, 64, 64, 16), (1, 64, 64, 32), (3, 64, 96, 32)])
def test_patch_rows_u8_equal_the_float_pack_bit_for_bit(lib, dtype, kind, B, H, W, patch):
    """32x48: 144 bytes per image row, so a wave's 16-pixel runs wrap rows inside one load; patch 32: a run is half a patch row."""
    ldt = DT[dtype][1]
    mean, std = IMAGENET if kind == "random" else HALF
    u8 = images_u8(B, H, W, seed=B + H, kind=kind)
    xf = to_tensor_normalize(u8, mean, std).cuda()
    n = B * (H // patch) * (W // patch) * 3 * patch * patch
    ref_buf, ref = guarded(n)
    got_buf, got = guarded(n)
    _lib.check(lib.lseg_op_patch_rows(P(xf), P(ref), B, H, W, patch, ldt, stream()))
    xd = u8.cuda()
    _lib.check(lib.lseg_op_patch_rows_u8(P(xd), P(got), B, H, W, patch, ldt, F3(mean), F3(std), stream()))
    torch.cuda.synchronize()
    assert not bool((ref == SENTINEL).all()) and guards_untouched(ref_buf, n)
    assert torch.equal(got, ref), f"{int((got != ref).sum())} of {n} words differ"
    assert guards_untouched(got_buf, n)


# ---- 2. op level: the ResNet-101 stem ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["bf16", "fp16"])
@pytest.mark.parametrize("kind", ["arange", "random"])
@pytest.mark.parametrize("B,H,W", [(1, 64, 64), (3, 64, 64), (1, 32, 96), (3, 32, 96), (2, 34, 70)])
def test_rn_stem_u8_equals_the_float_stem_bit_for_bit(lib, dtype, kind, B, H, W):
    """34x70: 35 output columns = two column tiles, the second nearly empty, and a buffer of 14 280 bytes -- no multiple of 16, so the
    last chunk of the image is the one read byte by byte."""
    ldt = DT[dtype][1]
    mean, std = IMAGENET if kind == "random" else HALF
    u8 = images_u8(B, H, W, seed=7 * B + W, kind=kind)
    xf = to_tensor_normalize(u8, mean, std).cuda()
    g = torch.Generator().manual_seed(3)
    w = (torch.randn((64, 3, 7, 7), generator=g) * math.sqrt(2 / 147)).reshape(64, 147).t().contiguous().cuda()
    bias = (torch.randn((64,), generator=g) * 0.1).cuda()
    n = B * (H // 2 + 2) * (W // 2 + 2) * 64
    ref_buf, ref = guarded(n)
    got_buf, got = guarded(n)
    _lib.check(lib.lseg_op_rn_stem(P(xf), P(w), P(bias), P(ref), B, H, W, ldt, stream()))
    xd = u8.cuda()
    _lib.check(lib.lseg_op_rn_stem_u8(P(xd), P(w), P(bias), P(got), B, H, W, ldt, F3(mean), F3(std), stream()))
    torch.cuda.synchronize()
    interior = ref.view(B, H // 2 + 2, W // 2 + 2, 64)[:, 1:-1, 1:-1]
    assert not bool((interior == SENTINEL).any())                  # the float stem wrote every interior pixel (the border is the caller's)
    assert torch.equal(got, ref), f"{int((got != ref).sum())} of {n} words differ"
    assert guards_untouched(got_buf, n) and guards_untouched(ref_buf, n)


# ---- 3. whole path: the three network kinds -------------------------------------------------------------------------------------------
def _engine(cfg, sd, tok, H, W, B, group=0, **kw):
    eng = HipEngine(cfg, H, W, max_batch=B, max_labels=tok.shape[0], **kw)
    eng.load_state_dict(sd)
    eng.set_tokens(tok, labels_per_image=group)
    return eng


def _all_outputs(eng, x):
    out = {"logits": eng.forward(x), "labels": eng.forward_labels(x), "low": eng.forward_lowres(x)}
    out.update({"conf_" + k: v for k, v in eng.forward_labels_conf(x).items()})
    torch.cuda.synchronize()
    return {k: v.clone() for k, v in out.items()}


def _same(a, b, what):
    assert a.keys() == b.keys()
    bad = [k for k in a if not torch.equal(a[k], b[k])]
    assert not bad, f"{what}: {bad} differ"


@pytest.mark.parametrize("net", ["vit_shared", "vit_grouped", "resnet101_grouped"])
def test_whole_forwards_from_uint8_equal_the_float_forwards(net):
    """forward / forward_labels / forward_labels_conf / forward_lowres with uint8 input == the same on the host-normalised tensor; then
    a float call on the engine that just read uint8 == a float call on a fresh engine: no format state leaks."""
    B, H, W = 2, 64, 64
    cfg = get_config("clip_resnet101" if net.startswith("resnet") else "tiny16")
    sd = {k: v.cuda() for k, v in synthetic_state_dict(cfg, seed=4).items()}
    group = 0 if net == "vit_shared" else 2
    K = 5 if group == 0 else B * group
    tok = synthetic_tokens([f"label{i}" for i in range(K)], cfg.text.vocab, cfg.text.ctx)
    mean, std = IMAGENET
    u8 = images_u8(B, H, W, seed=11)
    xf, xd = to_tensor_normalize(u8, mean, std).cuda(), u8.cuda()
    eng = _engine(cfg, sd, tok, H, W, B, group)
    eng.set_input_u8(True, mean, std)
    from_u8 = _all_outputs(eng, xd)
    eng.set_input_u8(False)
    after = _all_outputs(eng, xf)
    fresh = _all_outputs(_engine(cfg, sd, tok, H, W, B, group), xf)
    assert from_u8["logits"].shape == (B, K if group == 0 else group, H, W)
    _same(from_u8, fresh, "uint8 input vs float input")
    _same(after, fresh, "float call after a uint8 call vs a fresh engine")


def test_networks_switch_the_format_per_call():
    """LSegNet and LSegRNNetZS take a uint8 [B,H,W,3] batch where they take float [B,3,H,W]; a float call afterwards is unchanged."""
    from modules.models.lseg_net import LSegNet
    from modules.models.lseg_net_zs import LSegRNNetZS
    u8 = images_u8(2, 64, 64, seed=5)
    xf, xd = to_tensor_normalize(u8, *HALF).cuda(), u8.cuda()
    labels = ["wall", "sky", "tree", "floor", "other"]
    net = LSegNet(labels=labels, backbone="tiny16", features=get_config("tiny16").features, arch_option=0, block_depth=0, activation="lrelu")
    net.load_state_dict(synthetic_state_dict(net.cfg, seed=5))
    net = net.cuda().eval()
    with torch.no_grad():
        before = {"logits": net(xf).clone(), "labels": net.predict_labels(xf).clone(), "low": net.forward_lowres(xf).clone()}
        from_u8 = {"logits": net(xd).clone(), "labels": net.predict_labels(xd).clone(), "low": net.forward_lowres(xd).clone()}
        after = {"logits": net(xf).clone(), "labels": net.predict_labels(xf).clone(), "low": net.forward_lowres(xf).clone()}
    _same(from_u8, before, "LSegNet uint8 vs float")
    _same(after, before, "LSegNet float after uint8")
    rn = LSegRNNetZS(label_list=[f"class{i}" for i in range(10)], backbone="clip_resnet101", features=256, aux=False, use_pretrained=False,
                     arch_option=0, block_depth=0, activation="lrelu", image_dtype="fp16")
    rn.load_state_dict(synthetic_state_dict(get_config("clip_resnet101"), seed=5), strict=False)
    rn = rn.cuda().eval()
    with torch.no_grad():
        a, b, c = rn(xf, [3, 7]).clone(), rn(xd, [3, 7]).clone(), rn(xf, [3, 7]).clone()
    assert torch.equal(a, b) and torch.equal(a, c)


# ---- 4. train mode ------------------------------------------------------------------------------------------------------------------
def test_training_step_from_uint8_equals_the_float_step():
    """forward + backward(target=...) with deterministic reductions (flags bit 3): the loss and the gradients -- one scratch.* and one
    pretrained.* parameter named, all of them compared -- are the float route's bits."""
    B, H, W, K = 2, 64, 64, 5
    cfg = get_config("tiny16")
    sd = synthetic_state_dict(cfg, seed=3)
    tok = synthetic_tokens([f"label{i}" for i in range(K)], cfg.text.vocab, cfg.text.ctx)
    u8 = images_u8(B, H, W, seed=3)
    g = torch.Generator().manual_seed(1003)
    target = torch.randint(0, K, (B, H, W), generator=g)
    target[torch.rand((B, H, W), generator=g) < 0.2] = -1
    runs = {}
    for fmt in ("float", "u8"):
        sd_dev = {k: v.clone().cuda() for k, v in sd.items()}          # (train-mode BatchNorm moves the running statistics)
        eng = HipEngine(cfg, H, W, max_batch=B, max_labels=K, deterministic=True)
        eng.load_state_dict(sd_dev)
        eng.set_tokens(tok)
        eng.enable_training(sd_dev)
        if fmt == "u8":
            eng.set_input_u8(True, *IMAGENET)
            x = u8.cuda()
        else:
            x = to_tensor_normalize(u8, *IMAGENET).cuda()
        logits = eng.forward(x)
        loss = eng.backward(target=target.cuda(), ignore_index=-1)
        torch.cuda.synchronize()
        runs[fmt] = (logits.clone(), loss.clone(), {k: v.clone() for k, v in eng.grads.items()})
    (lf, lossf, gf), (lu, lossu, gu) = runs["float"], runs["u8"]
    assert torch.equal(lu, lf) and torch.equal(lossu, lossf), (float(lossu), float(lossf))
    for k in ("scratch.head1.weight", "pretrained.model.patch_embed.proj.weight"):
        assert k in gf and float(gf[k].abs().sum()) > 0 and torch.equal(gu[k], gf[k]), k
    assert not [k for k in gf if not torch.equal(gu[k], gf[k])]


# ---- 5. evaluator -------------------------------------------------------------------------------------------------------------------
def _crops_float(lib, xf, H, W, g, crop, flip, pad):
    cur = torch.empty((3, g.height, g.width), dtype=torch.float32, device="cuda")
    _lib.check(lib.lseg_op_eval_resize(P(xf), P(cur), 3, H, W, g.height, g.width, 0, stream()))
    crops = torch.full(((1 + flip) * g.n_box, 3, crop, crop), float("nan"), dtype=torch.float32, device="cuda")
    _lib.check(lib.lseg_op_eval_make_crops(P(cur), P(crops), 3, g.height, g.width, crop, g.stride, g.h_grids, g.w_grids, flip, pad, stream()))
    return crops


@pytest.mark.parametrize("flip", [1, 0])
@pytest.mark.parametrize("scale", [0.5, 0.75, 1.0, 1.5])
def test_eval_make_crops_u8_equals_resize_plus_make_crops(lib, scale, flip):
    """40x56 image, base 56, crop 32: scale 0.5 leaves the resized image (20x28) smaller than the crop both ways (one padded crop),
    0.75 (30x42) a 1x2 grid with padded rows, 1.0 a 2x3 grid, 1.5 (60x84) a 3x4 grid: rows and columns of boxes at stride 21, the last
    boxes reaching past the image."""
    H, W, crop, base = 40, 56, 32, 56
    mean, std = IMAGENET
    g = scale_geometry(H, W, scale, base, crop)
    if scale == 0.5:
        assert g.height < crop and g.width < crop and g.n_box == 1
    if scale == 1.5:
        assert g.h_grids >= 2 and g.w_grids >= 2
    u8 = images_u8(1, H, W, seed=9)[0]
    xf = to_tensor_normalize(u8, mean, std).cuda()
    pad = F3([-m / s for m, s in zip(mean, std)])
    ref = _crops_float(lib, xf, H, W, g, crop, flip, pad)
    n = ref.numel() * 2                                         # in 16-bit guard words
    buf, mid = guarded(n)
    got = mid.view(torch.float32).view(ref.shape)
    xd = u8.cuda()
    _lib.check(lib.lseg_op_eval_make_crops_u8(P(xd), P(got), H, W, g.height, g.width, crop, g.stride, g.h_grids, g.w_grids, flip, pad,
                                              F3(mean), F3(std), stream()))
    torch.cuda.synchronize()
    assert not bool(torch.isnan(ref).any())
    assert torch.equal(got.view(torch.int32), ref.view(torch.int32)), f"{int((got != ref).sum())} of {ref.numel()} values differ"
    assert guards_untouched(buf, n)


@pytest.mark.parametrize("lowres", [False, True])
def test_batched_multi_eval_takes_a_uint8_image(lowres):
    """BatchedMultiEval on one 40x56 uint8 image, crop 32, scales (0.75, 1.0, 1.5), flip: forward == the float call, bit for bit; the
    label route (forward_labels / parallel_*) takes the uint8 image too."""
    from modules.models.lseg_net import LSegNet
    H, W, K = 40, 56, 5
    labels = ["wall", "sky", "tree", "floor", "other"]
    net = LSegNet(labels=labels, backbone="tiny16", features=get_config("tiny16").features, arch_option=0, block_depth=0, activation="lrelu")
    net.load_state_dict(synthetic_state_dict(net.cfg, seed=6))
    net = net.cuda().eval()
    mean, std = IMAGENET
    ev = BatchedMultiEval(ModuleSurface(net, crop_size=32, base_size=56, mean=mean, std=std), K, flip=True, scales=(0.75, 1.0, 1.5), max_batch=8,
                          lowres=lowres)
    u8 = images_u8(1, H, W, seed=13)[0]
    xf = to_tensor_normalize(u8, mean, std)
    ref = ev.forward(xf.unsqueeze(0).cuda()).clone()
    got = ev.forward(u8.cuda()).clone()
    torch.cuda.synchronize()
    assert got.shape == (1, K, H, W) and torch.equal(got, ref)
    assert torch.equal(ev.parallel_forward([u8])[0], ref)
    if lowres:
        lab_f = ev.parallel_forward_labels([xf], confidence=True)[0]
        lab_u = ev.parallel_forward_labels([u8], confidence=True)[0]
        assert all(torch.equal(a, b) for a, b in zip(lab_u, lab_f))
        tgt = torch.randint(0, K, (H, W), generator=torch.Generator().manual_seed(1))
        mf, mu = ev.parallel_forward_metrics([xf], [tgt])[0], ev.parallel_forward_metrics([u8], [tgt])[0]
        assert mf.keys() == mu.keys() and all(torch.equal(torch.as_tensor(mf[k]), torch.as_tensor(mu[k])) for k in mf)


# ---- 6. refusals, each with its documented status -------------------------------------------------------------------------------------
def test_refusals_return_their_documented_status(lib):
    B, H, W, K = 1, 64, 64, 5
    cfg = get_config("tiny16")
    sd = {k: v.cuda() for k, v in synthetic_state_dict(cfg, seed=4).items()}
    tok = synthetic_tokens([f"label{i}" for i in range(K)], cfg.text.vocab, cfg.text.ctx)
    u8 = images_u8(B, H, W, seed=2).cuda()
    xf = to_tensor_normalize(u8.cpu(), *HALF).cuda()
    eng = _engine(cfg, sd, tok, H, W, B)

    def status(fn):
        with pytest.raises(_lib.LSegError) as e:
            fn()
        return e.value.code, str(e.value)

    code, msg = status(lambda: eng.forward(u8))                                  # uint8 without the format set
    assert code == -1 and "set_input_u8" in msg
    for bad in ((0.5, 0.0, 0.5), (0.5, float("nan"), 0.5)):                      # std = 0, non-finite: LSEG_ERR_INVALID, format unchanged
        assert status(lambda: eng.set_input_u8(True, HALF[0], bad))[0] == -1
        assert eng.input_u8 is None
    assert torch.equal(eng.forward(xf), _engine(cfg, sd, tok, H, W, B).forward(xf))          # ... and the float path still runs
    eng.set_input_u8(True, *HALF)
    code, msg = status(lambda: eng.forward(xf))                                  # float with the format set
    assert code == -1 and "set_input_u8(False)" in msg
    code, msg = status(lambda: eng.forward_labels(u8.permute(0, 3, 1, 2).contiguous()))      # [B,3,H,W] uint8: the wrong layout
    assert code == -1 and "HWC" in msg
    strict = HipEngine(cfg, H, W, max_batch=B, max_labels=K, image_dtype="strict")
    code, msg = status(lambda: strict.set_input_u8(True, *HALF))                 # split precision reads fp32 only
    assert code == -5 and "split-precision" in msg and strict.input_u8 is None
    m, s0 = F3(HALF[0]), F3((0.5, 0.5, 0.0))
    assert lib.lseg_set_input_u8(eng._h, 1, m, s0) == -1                         # the C entry itself, with a live handle
    assert lib.lseg_set_input_u8(strict._h, 1, m, m) == -5
    assert lib.lseg_set_input_u8(strict._h, 0, None, None) == 0


def test_unaligned_uint8_batch_is_copied_not_refused():
    """A contiguous uint8 batch that starts 8 bytes into its storage: the kernels load 16-byte chunks from the batch's first byte, so
    HipEngine hands over an aligned copy (same masks); the C entry, given the raw pointer, refuses it with LSEG_ERR_INVALID."""
    B, H, W, K = 1, 64, 64, 5
    cfg = get_config("tiny16")
    sd = {k: v.cuda() for k, v in synthetic_state_dict(cfg, seed=4).items()}
    tok = synthetic_tokens([f"label{i}" for i in range(K)], cfg.text.vocab, cfg.text.ctx)
    u8 = images_u8(B, H, W, seed=2).cuda()
    store = torch.zeros(8 + u8.numel(), dtype=torch.uint8, device="cuda")
    odd = store[8:].view(B, H, W, 3)
    odd.copy_(u8)
    assert odd.is_contiguous() and odd.data_ptr() % 16 == 8
    eng = _engine(cfg, sd, tok, H, W, B)
    eng.set_input_u8(True, *HALF)
    assert torch.equal(eng.forward_labels(odd), eng.forward_labels(u8))
    lab = torch.empty((B, H, W), dtype=torch.int16, device="cuda")
    assert eng.lib.lseg_forward_labels(eng._h, P(odd), B, P(lab), None, stream()) == -1
    assert "aligned" in eng.lib.lseg_last_error(None).decode()
    torch.cuda.synchronize()


def test_native_training_step_takes_both_formats_on_one_engine():
    """LSegmentationModule.native_training_step on the shared train engine: a float step after forward_loss(uint8) runs as before, and
    the step takes a uint8 batch itself -- the same loss as the float step of a twin module."""
    import warnings
    warnings.simplefilter("ignore")
    from test_gpu_train_dp import _TinyModule
    labels = ["wall", "sky", "tree", "floor", "other"]
    sd = synthetic_state_dict(get_config("tiny16"), seed=12)
    u8 = images_u8(2, 64, 64, seed=21)
    xf, xd = to_tensor_normalize(u8, *HALF).cuda(), u8.cuda()
    target = torch.randint(0, 5, (2, 64, 64), generator=torch.Generator().manual_seed(5)).cuda()
    ma, mb = _TinyModule.make(sd, labels), _TinyModule.make(sd, labels)
    la = [float(ma.native_training_step(xd, target)), float(ma.native_training_step(xf, target)), float(ma.native_training_step(xd, target))]
    lb = [float(mb.native_training_step(xf, target)) for _ in range(3)]
    # the gradients are bit-reproducible (deterministic reductions), the loss VALUE is a double-precision atomic sum whose order moves
    # its last bits (forward_request.hip, check_ragged_train's note): after the rounding to fp32 that is one ulp at the most
    assert all(abs(a - b) <= 2.0 ** -23 * abs(b) for a, b in zip(la, lb)), (la, lb)
    loss = ma.net.forward_loss(xd, target)               # leaves the engine in the uint8 format ...
    assert float(loss) > 0
    assert float(ma.native_training_step(xf, target)) > 0          # ... and the float step still runs
