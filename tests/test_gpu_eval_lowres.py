"""The multi-scale evaluator on the low-resolution logits (lseg_forward_lowres + lseg_op_eval_accumulate_lowres): the same bits as the
full-resolution path -- the op against lseg_op_eval_accumulate(upsample x2), forward_lowres against forward, BatchedMultiEval(lowres=True)
against BatchedMultiEval() -- with a quarter of the logits alive."""
import ctypes as C
import warnings

import pytest
import torch
import torch.nn.functional as F

pytestmark = [pytest.mark.gpu, pytest.mark.gpu_fast]

LABELS = ["wall", "sky", "tree", "floor", "other"]


def _P(t):
    return C.c_void_p(t.data_ptr())


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _upsample2x(low):
    """output_conv's x2 bilinear of [P, h, h] planes.  lseg_op_upsample2x_planes where it accepts the width (a multiple of 4); below that
    (crop 12: 6-wide planes) lseg_op_eval_resize, the generic align_corners=True resize on the same src_tap / bilerp helpers -- the two are
    held bit-equal in test_the_two_upsamplers_agree."""
    from lseg_hip import _lib
    lib = _lib.load()
    p, h, w = low.shape
    out = torch.empty((p, 2 * h, 2 * w), dtype=torch.float32, device=low.device)
    if w % 4 == 0:
        _lib.check(lib.lseg_op_upsample2x_planes(_P(low), _P(out), p, h, w, _stream()))
    else:
        _lib.check(lib.lseg_op_eval_resize(_P(low), _P(out), p, h, w, 2 * h, 2 * w, 0, _stream()))
    return out


# crop, stride, (h_grids, w_grids), (height, width), (ph, pw)
GEOMETRIES = {
    "overlap_clipped": (12, 8, (2, 3), (17, 26), (18, 27)),        # overlapping boxes; ph / pw clip the last box of each axis
    "one_box_cropped_back": (12, 8, (1, 1), (9, 7), (12, 12)),     # height, width < crop: the padded image cropped back
    "width_29": (16, 10, (2, 3), (25, 29), (26, 29)),              # width no multiple of 4, odd offsets x - w0 (29 columns need 3 boxes)
    "grids_3x2": (16, 10, (3, 2), (33, 23), (34, 26)),             # the 3 x 2 grid: at most 26 columns, 23 kept (odd, no multiple of 4)
    "crop_24": (24, 16, (2, 3), (37, 53), (40, 56)),               # 12-wide planes: the reference goes through lseg_op_upsample2x_planes
}


def _random_low(K, crop, n, flip, seed):
    g = torch.Generator().manual_seed(seed)
    return (torch.rand(((2 if flip else 1) * n, K, crop // 2, crop // 2), generator=g) * 2 - 1).cuda()


def _composition(low, K, geo, flip):
    from lseg_hip import _lib
    lib = _lib.load()
    crop, stride, (hg, wg), (height, width), (ph, pw) = geo
    full = _upsample2x(low.view(-1, crop // 2, crop // 2)).view(low.shape[0], K, crop, crop)
    out = torch.empty((K, height, width), dtype=torch.float32, device="cuda")
    _lib.check(lib.lseg_op_eval_accumulate(_P(full), _P(out), K, height, width, ph, pw, crop, stride, hg, wg, int(flip), _stream()))
    return out


def _lowres(low, K, geo, flip, out=None):
    from lseg_hip import _lib
    lib = _lib.load()
    crop, stride, (hg, wg), (height, width), (ph, pw) = geo
    if out is None:
        out = torch.empty((K, height, width), dtype=torch.float32, device="cuda")
    _lib.check(lib.lseg_op_eval_accumulate_lowres(_P(low), _P(out), K, height, width, ph, pw, crop, stride, hg, wg, int(flip), _stream()))
    return out


def test_the_two_upsamplers_agree():
    """lseg_op_eval_resize at exactly x2 is lseg_op_upsample2x_planes bit for bit (both are src_tap + bilerp): the stand-in used for the
    6-wide planes of crop 12 is the same function."""
    from lseg_hip import _lib
    lib = _lib.load()
    for h in (8, 12):
        low = (torch.rand((7, h, h), generator=torch.Generator().manual_seed(h)) * 2 - 1).cuda()
        a = torch.empty((7, 2 * h, 2 * h), device="cuda")
        b = torch.empty_like(a)
        _lib.check(lib.lseg_op_upsample2x_planes(_P(low), _P(a), 7, h, h, _stream()))
        _lib.check(lib.lseg_op_eval_resize(_P(low), _P(b), 7, h, h, 2 * h, 2 * h, 0, _stream()))
        assert torch.equal(a, b)


@pytest.mark.parametrize("flip", [0, 1])
@pytest.mark.parametrize("K", [1, 5])
@pytest.mark.parametrize("name", list(GEOMETRIES))
def test_accumulate_lowres_is_bit_identical_to_upsample_then_accumulate(name, K, flip):
    geo = GEOMETRIES[name]
    crop, _, (hg, wg), _, _ = geo
    low = _random_low(K, crop, hg * wg, flip, seed=3)
    want = _composition(low, K, geo, flip)
    got = _lowres(low, K, geo, flip)
    torch.cuda.synchronize()
    assert torch.isfinite(want).all()
    assert torch.equal(got, want), (got - want).abs().max().item()


@pytest.mark.parametrize("off", [1, 2, 3])
def test_accumulate_lowres_into_a_map_at_a_4_byte_aligned_offset(off):
    """d_map `off` floats into a 16-byte aligned allocation: the rows' 16-byte runs start elsewhere, the values do not change, and
    nothing outside the map is written."""
    geo, K = GEOMETRIES["width_29"], 5
    crop, _, (hg, wg), (height, width), _ = geo
    low = _random_low(K, crop, hg * wg, 1, seed=4)
    want = _composition(low, K, geo, 1)
    n = K * height * width
    buf = torch.full((n + 8,), 12345.0, device="cuda")
    assert buf.data_ptr() % 16 == 0
    view = buf[off:off + n].view(K, height, width)
    _lowres(low, K, geo, 1, out=view)
    torch.cuda.synchronize()
    assert torch.equal(view, want)
    assert (buf[:off] == 12345.0).all() and (buf[off + n:] == 12345.0).all()


def test_accumulate_lowres_equals_the_torch_statement():
    """The definition itself, on the CPU in fp32: F.interpolate x2 (align_corners=True), out + flip(twin), overlap-add in box order, count,
    divide, crop.  Bound: the operands are in [-1, 1); torch's source index and lambda are the kernel's (scale * index rounded, then the
    subtraction), so the two interpolations differ by their last roundings only, <= 2 ulp(1) = 2.4e-7 per value; up to 8 values (4 boxes x
    2) are summed and the sum divided by the 4 boxes: <= 8 x 2.4e-7 / 4 + the sums' own roundings (each side <= 0.5 ulp per add, adds at
    magnitudes <= 8: < 7 x 4.8e-7 / 4 in the worst case, typically a tenth of that) -- under 1e-6 for these shapes short of the worst
    case on every term at once."""
    name, K, flip = "overlap_clipped", 5, 1
    geo = GEOMETRIES[name]
    crop, stride, (hg, wg), (height, width), (ph, pw) = geo
    n = hg * wg
    low = _random_low(K, crop, n, flip, seed=5)
    got = _lowres(low, K, geo, flip).cpu()
    up = F.interpolate(low.cpu(), scale_factor=2, mode="bilinear", align_corners=True)
    outs = up[:n] + torch.flip(up[n:], dims=[3])
    acc = torch.zeros((K, ph, pw))
    cnt = torch.zeros((1, ph, pw))
    for idh in range(hg):
        for idw in range(wg):
            h0, w0 = idh * stride, idw * stride
            h1, w1 = min(h0 + crop, ph), min(w0 + crop, pw)
            acc[:, h0:h1, w0:w1] += outs[idh * wg + idw, :, :h1 - h0, :w1 - w0]
            cnt[:, h0:h1, w0:w1] += 1
    want = (acc / cnt)[:, :height, :width]
    d = (got - want).abs().max().item()
    print(f"accumulate_lowres vs torch statement: max |d| = {d:.3e}")
    assert d <= 1e-6, d


# ---- forward_lowres ---------------------------------------------------------------------------------------------------------------
def _net(image_dtype=None, arch_option=0, block_depth=0, seed=2):
    from lseg_hip.config import get_config
    from lseg_hip.synth import synthetic_state_dict
    from modules.models.lseg_net import LSegNet
    cfg = get_config("tiny16", arch_option=arch_option, block_depth=block_depth, activation="lrelu")
    kw = {} if image_dtype is None else {"image_dtype": image_dtype}
    net = LSegNet(labels=LABELS, backbone="tiny16", features=cfg.features, arch_option=arch_option, block_depth=block_depth,
                  activation="lrelu", batch_invariant=True, **kw)
    net.load_state_dict(synthetic_state_dict(cfg, seed=seed))
    return net.eval().cuda()


def _up_logits(low):
    b, k, h, w = low.shape
    return _upsample2x(low.reshape(b * k, h, w)).view(b, k, 2 * h, 2 * w)


@pytest.mark.parametrize("image_dtype", ["bf16", None])
def test_forward_lowres_upsampled_is_forward(image_dtype):
    warnings.simplefilter("ignore")
    from lseg_hip import metrics
    from lseg_hip.synth import synthetic_images
    net = _net(image_dtype)
    x = synthetic_images(3, 64, 64, seed=7).cuda()
    with torch.no_grad():
        want = net(x)
        low = net.forward_lowres(x)
        assert low.shape == (3, 5, 32, 32) and low.dtype == torch.float32
        assert torch.equal(_up_logits(low), want)
        # the engine is in the state an ordinary forward leaves: forward_stats reads the same logits
        g = torch.Generator().manual_seed(1)
        target = torch.randint(0, 5, (3, 64, 64), generator=g)
        target[torch.rand((3, 64, 64), generator=g) < 0.25] = -1
        fused = net._last_engine.forward_stats(target.cuda())
        full = metrics.seg_stats(want, target.cuda())
        for k in ("correct", "labeled", "nll_count"):
            assert full[k] == fused[k], k
        for k in ("area_inter", "area_pred", "area_lab", "area_union"):
            assert torch.equal(full[k], fused[k]), k
        assert abs(full["nll_sum"] - fused["nll_sum"]) <= 1e-6 * abs(full["nll_sum"])      # the same fp64 terms in another order
        # ... and so does the "lowres" tap
        assert torch.equal(net._last_engine.intermediate("lowres", low.shape), low)
        # a label subset
        sub = LABELS[1:4]
        want_s = net(x, sub)
        low_s = net.forward_lowres(x, sub)
        assert low_s.shape == (3, 3, 32, 32)
        assert torch.equal(_up_logits(low_s), want_s)


def test_forward_lowres_with_head_blocks():
    warnings.simplefilter("ignore")
    from lseg_hip.synth import synthetic_images
    net = _net(arch_option=1, block_depth=2)
    x = synthetic_images(3, 64, 64, seed=8).cuda()
    with torch.no_grad():
        want = net(x)
        low = net.forward_lowres(x)
        assert torch.equal(_up_logits(low), want)


def test_forward_lowres_raises_in_train_mode():
    warnings.simplefilter("ignore")
    from lseg_hip import _lib
    from lseg_hip.synth import synthetic_images
    net = _net("bf16")                                 # the engine's train mode needs bf16 operands
    x = synthetic_images(1, 64, 64, seed=9).cuda()
    with torch.no_grad():
        net.forward_lowres(x)
    eng = net._last_engine
    net.train()
    try:
        with pytest.raises(RuntimeError):
            net.forward_lowres(x)                      # the network refuses under net.train() with grad enabled ...
    finally:
        net.eval()
    eng.set_train(True)                                # ... and the engine itself in train mode: LSEG_ERR_UNSUPPORTED
    try:
        with pytest.raises(_lib.LSegError) as e:
            eng.forward_lowres(x)
        assert e.value.code == -5
    finally:
        eng.set_train(False)
    with pytest.raises(_lib.LSegError) as e:           # a NULL output
        _lib.check(eng.lib.lseg_forward_lowres(eng._h, _P(x), 1, None, _stream()))
    assert e.value.code == -1


# ---- the whole evaluator -------------------------------------------------------------------------------------------------------------
class _Mod(torch.nn.Module):
    def __init__(self, net, crop, base):
        super().__init__()
        self.net, self.crop_size, self.base_size = net, crop, base
        self.mean, self.std = [0.5] * 3, [0.5] * 3
        self._up_kwargs = {"mode": "bilinear", "align_corners": True}

    def evaluate(self, x, target=None):
        return self.net(x)

    def evaluate_random(self, x, labelset, target=None):
        return self.net(x, labelset)

    def evaluate_lowres(self, x):
        return self.net.forward_lowres(x)

    def evaluate_random_lowres(self, x, labelset):
        return self.net.forward_lowres(x, labelset)


@pytest.mark.parametrize("image_dtype", ["bf16", None])
def test_lowres_evaluator_is_bit_identical_and_holds_less_memory(image_dtype):
    """80 x 104 image, crop 64, base 72, six scales + flip, max_batch 8 (the setup of the sequential-schedule test): the scores of the
    low-resolution path are the default path's bit for bit, whatever max_stack groups the crops into, for the module's own labels and
    for a label subset; and its peak memory is lower."""
    warnings.simplefilter("ignore")
    from lseg_hip.evaluator import BatchedMultiEval
    from lseg_hip.synth import synthetic_images
    mod = _Mod(_net(image_dtype), crop=64, base=72)
    img = synthetic_images(1, 80, 104, seed=5).cuda()
    scales = [0.5, 0.75, 1.0, 1.25, 1.5, 1.75]
    full = BatchedMultiEval(mod, len(LABELS), flip=True, scales=scales, max_batch=8)
    lowr = BatchedMultiEval(mod, len(LABELS), flip=True, scales=scales, max_batch=8, lowres=True)
    with torch.no_grad():
        full(img); lowr(img)                            # engines, text features and the allocator's pools exist before the peaks are read
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        want = full(img)
        torch.cuda.synchronize()
        peak_full = torch.cuda.max_memory_allocated()
        torch.cuda.reset_peak_memory_stats()
        got = lowr(img)
        torch.cuda.synchronize()
        peak_low = torch.cuda.max_memory_allocated()
        assert got.shape == want.shape == (1, 5, 80, 104)
        assert torch.equal(got, want), (got - want).abs().max().item()
        print(f"peak memory allocated: default {peak_full} B, lowres {peak_low} B")
        assert peak_low < peak_full, (peak_low, peak_full)
        for max_stack in (6, 20):                      # several stacks / scales sharing a stack; the default (192) was one stack
            lowr.max_stack = max_stack
            assert torch.equal(lowr(img), want), max_stack
        del lowr.max_stack
        sub_want = full.parallel_forward([img[0]], label_set=LABELS[:3])
        sub_got = lowr.parallel_forward([img[0]], label_set=LABELS[:3])
        assert sub_got[0].shape == (1, 3, 80, 104)
        assert torch.equal(sub_got[0], sub_want[0])
