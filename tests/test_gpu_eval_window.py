"""A scale of the multi-scale evaluator in WINDOWS of its crop grid (lseg_op_eval_accumulate_window / _window_lowres + lseg_op_eval_finalize):
any partition of the grid, submitted in ascending order, leaves the bits of the one-launch kernels; a window touches only its footprint;
BatchedMultiEval splits a scale that does not fit in max_stack and leaves every other scale on the path it had."""
import ctypes as C
import warnings

import pytest
import torch

pytestmark = [pytest.mark.gpu, pytest.mark.gpu_fast]

LSEG_ERR_INVALID = -1
LABELS = ["wall", "sky", "tree", "floor", "other"]
SENTINEL = 12345.0


def _P(t):
    return C.c_void_p(t.data_ptr())


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _lib_():
    from lseg_hip import _lib
    return _lib, _lib.load()


# K, crop, stride, (h_grids, w_grids), (height, width), (ph, pw)
K, CROP, STRIDE = 3, 8, 5
GEOMETRIES = {
    "19x14": ((4, 3), (19, 14), (19, 14)),           # pixels under 1, 2 and 4 boxes; the overlaps straddle windows
    "19x6_one_column": ((4, 1), (19, 6), (19, 8)),   # narrower than a crop: padded to pw = 8, one column of boxes, cropped back to 6
    "19x6_idle_columns": ((4, 3), (19, 6), (19, 8)),  # the 4 x 3 grid over that map: the boxes of columns 1, 2 lie (partly) in the padding
}
PARTITIONS = {12: [(12,), (1,) * 12, (5, 5, 2), (7, 5)], 4: [(4,), (1,) * 4, (2, 1, 1), (3, 1)]}
CASES = [(name, part) for name, g in GEOMETRIES.items() for part in PARTITIONS[g[0][0] * g[0][1]]]


def _logits(n, flip, side, seed):
    g = torch.Generator().manual_seed(seed)
    return (torch.rand(((2 if flip else 1) * n, K, side, side), generator=g) * 2 - 1).cuda()


def _one_launch(outs, geo, flip, lowres=False):
    _lib, lib = _lib_()
    (hg, wg), (height, width), (ph, pw) = geo
    out = torch.empty((K, height, width), dtype=torch.float32, device="cuda")
    fn = lib.lseg_op_eval_accumulate_lowres if lowres else lib.lseg_op_eval_accumulate
    _lib.check(fn(_P(outs), _P(out), K, height, width, ph, pw, CROP, STRIDE, hg, wg, int(flip), _stream()))
    return out


def _gather(outs, n, first, nb, flip):
    """The logits of boxes [first, first + nb) and, behind them, of their twins: what a forward of that window's crops returns."""
    return (torch.cat([outs[first:first + nb], outs[n + first:n + first + nb]], dim=0) if flip else outs[first:first + nb]).contiguous()


def _one_float_past_16_bytes(t):
    """The same values in memory that starts 4 bytes past a 16-byte boundary."""
    buf = torch.empty(t.numel() + 4, dtype=t.dtype, device=t.device)
    view = buf[1:1 + t.numel()].view(t.shape)
    view.copy_(t)
    assert view.data_ptr() % 16 == 4 and view.is_contiguous()
    return view


def _windowed(outs, geo, flip, part, lowres=False, in_place=True, misalign=False):
    _lib, lib = _lib_()
    (hg, wg), (height, width), (ph, pw) = geo
    n = hg * wg
    assert sum(part) == n
    fn = lib.lseg_op_eval_accumulate_window_lowres if lowres else lib.lseg_op_eval_accumulate_window
    ssum = torch.zeros((K, height, width), dtype=torch.float32, device="cuda")
    first = 0
    for nb in part:
        win = _gather(outs, n, first, nb, flip)
        if misalign:
            win = _one_float_past_16_bytes(win)
        _lib.check(fn(_P(win), _P(ssum), K, height, width, ph, pw, CROP, STRIDE, hg, wg, int(flip), first, nb, _stream()))
        first += nb
    out = ssum if in_place else torch.empty_like(ssum)
    _lib.check(lib.lseg_op_eval_finalize(_P(ssum), _P(out), K, height, width, ph, pw, CROP, STRIDE, hg, wg, _stream()))
    return out


def _upsample2x(low):
    _lib, lib = _lib_()
    n, k, h, w = low.shape
    out = torch.empty((n, k, 2 * h, 2 * w), dtype=torch.float32, device="cuda")
    _lib.check(lib.lseg_op_upsample2x_planes(_P(low), _P(out), n * k, h, w, _stream()))
    return out


@pytest.mark.parametrize("flip", [0, 1])
@pytest.mark.parametrize("name,part", CASES)
def test_windows_then_finalize_are_the_one_launch_kernel_bit_for_bit(name, part, flip):
    geo = GEOMETRIES[name]
    outs = _logits(geo[0][0] * geo[0][1], flip, CROP, seed=11)
    want = _one_launch(outs, geo, flip)
    got = _windowed(outs, geo, flip, part, in_place=len(part) % 2 == 0)       # finalize in place and into another buffer
    torch.cuda.synchronize()
    assert torch.isfinite(want).all()
    assert torch.equal(got, want), (got - want).abs().max().item()


@pytest.mark.parametrize("flip", [0, 1])
@pytest.mark.parametrize("name,part", CASES)
def test_lowres_windows_equal_the_lowres_kernel_and_the_full_resolution_windows(name, part, flip):
    geo = GEOMETRIES[name]
    low = _logits(geo[0][0] * geo[0][1], flip, CROP // 2, seed=12)             # [.., 4, 4] planes
    got = _windowed(low, geo, flip, part, lowres=True)
    want_lowres = _one_launch(low, geo, flip, lowres=True)
    want_full = _windowed(_upsample2x(low), geo, flip, part)
    torch.cuda.synchronize()
    assert torch.equal(got, want_lowres), (got - want_lowres).abs().max().item()
    assert torch.equal(got, want_full), (got - want_full).abs().max().item()


@pytest.mark.parametrize("lowres", [False, True])
@pytest.mark.parametrize("flip", [0, 1])
def test_windows_on_logits_one_float_past_a_16_byte_boundary(flip, lowres):
    """Every window's logits start 4 bytes past a 16-byte boundary: the full-resolution box reads its four consecutive logits (and the
    twin's) with four 4-byte loads wherever the address is not a multiple of 16, the low-resolution taps read unaligned rows.  The same
    bits as the one-launch entry on an aligned copy of the values (the tests above move the sum's alignment, not the logits')."""
    geo = GEOMETRIES["19x14"]
    outs = _logits(geo[0][0] * geo[0][1], flip, CROP // 2 if lowres else CROP, seed=15)
    want = _one_launch(outs, geo, flip, lowres=lowres)
    got = _windowed(outs, geo, flip, (5, 5, 2), lowres=lowres, misalign=True)
    torch.cuda.synchronize()
    assert torch.isfinite(want).all()
    assert torch.equal(got, want), (got - want).abs().max().item()


def _footprint(geo, first, nb):
    (hg, wg), (height, width), _ = geo
    m = torch.zeros((height, width), dtype=torch.bool)
    for b in range(first, first + nb):
        h0, w0 = (b // wg) * STRIDE, (b % wg) * STRIDE
        m[h0:h0 + CROP, w0:w0 + CROP] = True
    return m.cuda()


@pytest.mark.parametrize("lowres", [False, True])
@pytest.mark.parametrize("off", [0, 1])
@pytest.mark.parametrize("first,nb", [(0, 1), (4, 1), (11, 1), (2, 5), (5, 2)])
def test_a_window_touches_only_its_footprint(first, nb, off, lowres):
    """d_sum filled with a sentinel (and, off = 1, starting one float into the allocation, so that its rows' 16-byte runs start
    elsewhere): after one window every pixel outside the window's boxes still holds the sentinel's bits, every pixel inside holds
    sentinel + the window's boxes in order, and nothing around the map is written."""
    _lib, lib = _lib_()
    name, flip = "19x14", 1
    geo = GEOMETRIES[name]
    (hg, wg), (height, width), (ph, pw) = geo
    n = hg * wg
    side = CROP // 2 if lowres else CROP
    outs = _logits(n, flip, side, seed=13)
    total = K * height * width
    buf = torch.full((total + 8,), SENTINEL, device="cuda")
    ssum = buf[off:off + total].view(K, height, width)
    fn = lib.lseg_op_eval_accumulate_window_lowres if lowres else lib.lseg_op_eval_accumulate_window
    _lib.check(fn(_P(_gather(outs, n, first, nb, flip)), _P(ssum), K, height, width, ph, pw, CROP, STRIDE, hg, wg, flip, first, nb, _stream()))
    torch.cuda.synchronize()
    inside = _footprint(geo, first, nb)
    sent_bits = torch.full((1,), SENTINEL).view(torch.int32).item()
    assert (ssum.view(torch.int32)[:, ~inside] == sent_bits).all()
    assert (buf[:off] == SENTINEL).all() and (buf[off + total:] == SENTINEL).all()
    # inside: the sentinel plus out + flip(twin) of the covering boxes of the window, ascending
    full = _upsample2x(outs) if lowres else outs
    want = torch.full((K, height, width), SENTINEL, device="cuda")
    for b in range(first, first + nb):
        h0, w0 = (b // wg) * STRIDE, (b % wg) * STRIDE
        h1, w1 = min(h0 + CROP, height), min(w0 + CROP, width)
        v = full[b] + torch.flip(full[n + b], dims=[2])
        want[:, h0:h1, w0:w1] += v[:, :h1 - h0, :w1 - w0]
    assert torch.equal(ssum, want)
    assert (ssum[:, inside] != SENTINEL).any()


@pytest.mark.parametrize("name", ["lseg_op_eval_accumulate_window", "lseg_op_eval_accumulate_window_lowres"])
def test_bad_arguments_return_invalid_and_leave_the_sum_untouched(name):
    _lib, lib = _lib_()
    (hg, wg), (height, width), (ph, pw) = GEOMETRIES["19x14"]
    lowres = name.endswith("lowres")
    outs = _logits(hg * wg, 1, CROP // 2 if lowres else CROP, seed=14)
    ssum = torch.full((K, height, width), SENTINEL, device="cuda")
    fn = getattr(lib, name)

    def call(o=outs, s=ssum, crop=CROP, first=0, nb=2, hg_=hg):
        return fn(None if o is None else _P(o), None if s is None else _P(s), K, height, width, ph, pw, crop, STRIDE, hg_, wg, 1, first, nb,
                  _stream())
    assert call(o=None) == LSEG_ERR_INVALID
    assert call(s=None) == LSEG_ERR_INVALID
    assert call(nb=0) == LSEG_ERR_INVALID
    assert call(first=11, nb=2) == LSEG_ERR_INVALID          # boxes [11, 13) of a 12-box grid
    assert call(first=12, nb=1) == LSEG_ERR_INVALID
    assert call(hg_=3) == LSEG_ERR_INVALID                   # three rows of boxes end at 18 < 19
    if lowres:
        assert call(crop=9) == LSEG_ERR_INVALID              # odd: no crop/2 planes (9 still covers the map)
    assert lib.lseg_op_eval_finalize(None, _P(ssum), K, height, width, ph, pw, CROP, STRIDE, hg, wg, _stream()) == LSEG_ERR_INVALID
    assert lib.lseg_op_eval_finalize(_P(ssum), None, K, height, width, ph, pw, CROP, STRIDE, hg, wg, _stream()) == LSEG_ERR_INVALID
    assert lib.lseg_op_eval_finalize(_P(ssum), _P(ssum), K, height, width, ph, pw, CROP, STRIDE, 3, wg, _stream()) == LSEG_ERR_INVALID
    torch.cuda.synchronize()
    assert (ssum.view(torch.int32) == torch.full((1,), SENTINEL).view(torch.int32).item()).all()


# ---- the whole evaluator -------------------------------------------------------------------------------------------------------------
SCALES = [0.5, 1.0, 1.75]       # 80 x 104 image, crop 64 / base 72: 1 box, 1 x 2 boxes, 2 x 3 boxes (12 crops with their twins)


def _net(seed=2):
    from lseg_hip.config import get_config
    from lseg_hip.synth import synthetic_state_dict
    from modules.models.lseg_net import LSegNet
    cfg = get_config("tiny16")
    net = LSegNet(labels=LABELS, backbone="tiny16", features=cfg.features, arch_option=0, block_depth=0, activation="lrelu",
                  batch_invariant=True, image_dtype="bf16")
    net.load_state_dict(synthetic_state_dict(cfg, seed=seed))
    return net.eval().cuda()


class _Mod(torch.nn.Module):
    """The module surface of tests/test_gpu_evaluator.py with the low-resolution pair, counting the crops of every evaluate* call."""

    def __init__(self, net, crop, base):
        super().__init__()
        self.net, self.crop_size, self.base_size = net, crop, base
        self.mean, self.std = [0.5] * 3, [0.5] * 3
        self._up_kwargs = {"mode": "bilinear", "align_corners": True}
        self.calls = []

    def evaluate(self, x, target=None):
        self.calls.append(x.shape[0])
        return self.net(x)

    def evaluate_random(self, x, labelset, target=None):
        self.calls.append(x.shape[0])
        return self.net(x, labelset)

    def evaluate_lowres(self, x):
        self.calls.append(x.shape[0])
        return self.net.forward_lowres(x)

    def evaluate_random_lowres(self, x, labelset):
        self.calls.append(x.shape[0])
        return self.net.forward_lowres(x, labelset)


@pytest.fixture(scope="module")
def mod():
    warnings.simplefilter("ignore")
    return _Mod(_net(), crop=64, base=72)


@pytest.fixture(scope="module")
def img():
    from lseg_hip.synth import synthetic_images
    return synthetic_images(1, 80, 104, seed=5).cuda()


def _per_scale_scores(mod, img, label_set, flip=True):
    """The schedule as it stood before windows, one scale at a time with the one-launch kernels: resize, make_crops, one stack through the
    network, lseg_op_eval_accumulate, resize-add.  Crops are independent in the batch-invariant engine, so any grouping gives these bits."""
    from lseg_hip.evaluator import scale_geometry
    _lib, lib = _lib_()
    _, ch, h, w = img.shape
    crop = mod.crop_size
    nclass = len(LABELS) if label_set is None else len(label_set)
    pad = (C.c_float * 3)(-1.0, -1.0, -1.0)                    # -mean / std
    scores = torch.zeros((1, nclass, h, w), device="cuda")
    for scale in SCALES:
        height, width, ph, pw, hg, wg, stride = scale_geometry(h, w, scale, mod.base_size, crop)
        cur = torch.empty((ch, height, width), device="cuda")
        _lib.check(lib.lseg_op_eval_resize(_P(img), _P(cur), ch, h, w, height, width, 0, _stream()))
        crops = torch.empty(((2 if flip else 1) * hg * wg, ch, crop, crop), device="cuda")
        _lib.check(lib.lseg_op_eval_make_crops(_P(cur), _P(crops), ch, height, width, crop, stride, hg, wg, int(flip), pad, _stream()))
        outs = (mod.net(crops) if label_set is None else mod.net(crops, label_set)).contiguous()
        smap = torch.empty((nclass, height, width), device="cuda")
        _lib.check(lib.lseg_op_eval_accumulate(_P(outs), _P(smap), nclass, height, width, ph, pw, crop, stride, hg, wg, int(flip), _stream()))
        _lib.check(lib.lseg_op_eval_resize(_P(smap), _P(scores), nclass, height, width, h, w, 1, _stream()))
    return scores


@pytest.mark.parametrize("label_set", [None, LABELS[1:4]])
@pytest.mark.parametrize("lowres", [False, True])
def test_a_scale_larger_than_max_stack_runs_in_windows_with_the_same_scores(mod, img, lowres, label_set):
    from lseg_hip.evaluator import BatchedMultiEval, scale_geometry
    assert max(g[4] * g[5] for g in (scale_geometry(80, 104, s, 72, 64) for s in SCALES)) >= 6
    nclass = len(LABELS)
    small = BatchedMultiEval(mod, nclass, flip=True, scales=SCALES, max_batch=8, lowres=lowres, max_stack=4)
    large = BatchedMultiEval(mod, nclass, flip=True, scales=SCALES, max_batch=8, lowres=lowres, max_stack=64)
    groups = []
    inner = small._module_eval
    small._module_eval = lambda xs, ls: (groups.append(xs.shape[0]), inner(xs, ls))[1]
    with torch.no_grad():
        want = large(img, label_set)
        mod.calls.clear()
        got = small(img, label_set)
        calls = list(mod.calls)
        torch.cuda.synchronize()
        assert got.shape == (1, nclass if label_set is None else 3, 80, 104)
        assert sum(calls) == sum(groups) == 2 + 4 + 12                     # every crop and twin exactly once
        assert max(calls) <= 4, calls                                      # no forward beyond max_stack (and max_batch)
        assert max(groups) <= 4, groups                                    # no group's logits beyond max_stack crops
        assert torch.equal(got, want), (got - want).abs().max().item()
        assert torch.equal(got, _per_scale_scores(mod, img, label_set))


EVAL_ENTRIES = ["lseg_op_eval_resize", "lseg_op_eval_make_crops", "lseg_op_eval_accumulate", "lseg_op_eval_accumulate_lowres",
                "lseg_op_eval_accumulate_window", "lseg_op_eval_accumulate_window_lowres", "lseg_op_eval_finalize"]


def _record(monkeypatch):
    _lib, lib = _lib_()
    seq = []
    for name in EVAL_ENTRIES:
        fn = getattr(lib, name)
        monkeypatch.setattr(lib, name, lambda *a, _fn=fn, _name=name: (seq.append(_name), _fn(*a))[1])
    return seq


def test_scales_that_fit_use_none_of_the_window_entries(mod, img, monkeypatch):
    from lseg_hip.evaluator import BatchedMultiEval
    ev = BatchedMultiEval(mod, len(LABELS), flip=True, scales=SCALES, max_batch=8)      # default max_stack: 48
    seq = _record(monkeypatch)
    with torch.no_grad():
        got = ev(img)
    monkeypatch.undo()
    assert seq == ["lseg_op_eval_resize", "lseg_op_eval_make_crops"] * 3 + ["lseg_op_eval_accumulate", "lseg_op_eval_resize"] * 3, seq
    with torch.no_grad():
        assert torch.equal(got, _per_scale_scores(mod, img, None))
    # ... and the windowed call is made of the new ones for the large scale only
    ev = BatchedMultiEval(mod, len(LABELS), flip=True, scales=SCALES, max_batch=8, max_stack=4)
    seq = _record(monkeypatch)
    with torch.no_grad():
        ev(img)
    monkeypatch.undo()
    assert seq.count("lseg_op_eval_accumulate") == 2 and seq.count("lseg_op_eval_accumulate_window") == 3
    assert seq.count("lseg_op_eval_finalize") == 1 and seq.count("lseg_op_eval_make_crops") == 3


def test_the_engine_is_built_once_in_a_call_with_uneven_stacks(img, monkeypatch):
    """Stacks of 2, 4 and 3 x 4 crops: the network learns the largest forward before the first, so its engine is built once rather than
    closed and rebuilt when the second stack is larger than the first."""
    warnings.simplefilter("ignore")
    import lseg_hip.engine as E
    from lseg_hip.evaluator import BatchedMultiEval
    built = []

    class Counting(E.HipEngine):
        def __init__(self, *a, **kw):
            built.append(kw.get("max_batch"))
            super().__init__(*a, **kw)

    monkeypatch.setattr(E, "HipEngine", Counting)
    m = _Mod(_net(), crop=64, base=72)
    ev = BatchedMultiEval(m, len(LABELS), flip=True, scales=SCALES, max_batch=8, max_stack=4)
    with torch.no_grad():
        ev(img)
        torch.cuda.synchronize()
    assert m.calls == [2, 4, 4, 4, 4]
    assert built == [4], built
