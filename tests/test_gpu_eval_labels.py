"""Multi-scale masks for any label set (BatchedMultiEval.forward_labels): the merge kernel against the stable sort of the concatenated
planes, the held-feature entries of the engine against forward_lowres, and the evaluator's label panels against the stable sort of
BatchedMultiEval(lowres=True).forward's scores -- bit for bit wherever the two run the same arithmetic (K > 157)."""
import ctypes as C
import warnings

import numpy as np
import pytest
import torch

from eval_labels_helpers import PARTITIONS, merge_partition, planted_planes, stable_sort_reference

pytestmark = [pytest.mark.gpu, pytest.mark.gpu_fast]

LABELS = ["wall", "sky", "tree", "floor", "other"]
MANY = [f"thing number {i}" for i in range(160)]               # 160 distinct labels: above the 157 the fused correlation kernel holds
SHAPES = [(5, 7), (9, 261)]                                     # a partial run only; more runs than a wave's lanes per row, odd tail
ERR_INVALID, ERR_STATE, ERR_UNSUPPORTED = -1, -4, -5

# Largest |forward_lowres by default - forward_lowres under LSEG_CORR_GENERIC=1| over the logits of the engine test's K = 5 input (tiny16,
# seed 2, synthetic_images(3, 64, 64, seed=7), the labels above), each route in a fresh interpreter, on the parent commit.  Measured: 0
# for both operand types, 0 of 15 360 logits differ (and 0 over the evaluator test's scores): tiny16's out_c is 128, a width the fused
# kernel does not take, so both "routes" are the pixel_gram + generic GEMM pair there.  The tolerance is twice that: exact equality.
ROUTE_DIFF = {"bf16": 0.0, None: 0.0}


def _P(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


# ---- the op ----------------------------------------------------------------------------------------------------------------------------
def _merge(planes, partition, conf=True, off=0):
    """planes torch [K, H, W] on the device, submitted panel by panel; off: every buffer starts `off` floats (int16: `off` elements) into
    its 16-byte aligned allocation.  Returns the five outputs (None where not asked for) and the guard regions' verdict."""
    from lseg_hip import _lib
    lib = _lib.load()
    K, H, W = planes.shape
    n = H * W

    def buf(dtype, fill):
        b = torch.full((n + 8,), fill, dtype=dtype, device="cuda")
        assert b.data_ptr() % 16 == 0
        return b

    src = torch.full((K * n + 8,), 777.0, device="cuda")       # the planes too sit at the offset
    src[off:off + K * n] = planes.reshape(-1)
    pl = src[off:off + K * n].view(K, H, W)
    names = ("label", "score", "label2", "score2", "lse")
    bufs = {"label": buf(torch.int16, 77), "score": buf(torch.float32, 777.0)}
    if conf:
        bufs.update(label2=buf(torch.int16, 77), score2=buf(torch.float32, 777.0), lse=buf(torch.float32, 777.0))
    view = {k: b[off:off + n] for k, b in bufs.items()}
    row0 = 0
    for i, rows in enumerate(partition):
        _lib.check(lib.lseg_op_eval_merge_labels(_P(pl[row0:row0 + rows]), rows, row0, H, W, *(_P(view.get(k)) for k in names),
                                                 int(i == 0), int(i == len(partition) - 1), _stream()))
        row0 += rows
    torch.cuda.synchronize()
    clean = all((b[:off] == (77 if b.dtype == torch.int16 else 777.0)).all() and (b[off + n:] == (77 if b.dtype == torch.int16 else 777.0)).all()
                for b in bufs.values())
    return [view[k].view(H, W).cpu() if k in view else None for k in names], clean


def _op_cases():
    return [(shape, K, part) for shape in SHAPES for K, parts in PARTITIONS.items() for part in parts]


@pytest.fixture(scope="module")
def lse_bound():
    """4 x the largest error of the fp32 recurrence itself (the numpy restatement in np.float32 on the CPU: the kernel's arithmetic with
    the host's exp / log) against torch.logsumexp in fp64, over every input of the op test.  The device's exp / log differ from the
    host's by a few ulp: 4 x."""
    worst = 0.0
    for (H, W), K, part in _op_cases():
        planes = planted_planes(K, H, W, K, part)
        lse32 = merge_partition(planes.numpy(), part, np.float32)[4]
        worst = max(worst, float(np.abs(lse32.astype(np.float64) - stable_sort_reference(planes)[4].numpy()).max()))
    print(f"fp32 recurrence vs fp64 logsumexp over the op test's inputs: max |d| = {worst:.3e}; the kernel is allowed {4 * worst:.3e}")
    assert 0.0 < worst < 1e-5
    return 4.0 * worst


def _case_id(case):
    (H, W), K, part = case
    return f"{H}x{W}-K{K}-" + ("whole" if len(part) == 1 else "ones" if all(r == 1 for r in part) else "_".join(map(str, part)))


@pytest.mark.parametrize("shape,K,partition", _op_cases(), ids=[_case_id(c) for c in _op_cases()])
def test_merge_labels_equals_the_stable_sort_of_the_concatenated_planes(shape, K, partition, lse_bound):
    """rand * 2 - 1 planes with planted ties (inside a panel, across panels, a later plane equal to the winner): label / score / label2 /
    score2 are entries 0 / 1 of torch.sort(descending, stable) bit for bit for every partition; lse against torch.logsumexp in fp64 within
    4 x the fp32 recurrence's own error on these inputs (measured on the CPU over all cases of this test: 4.94e-07, so 1.98e-06 is
    allowed; the fixture recomputes it); the all-NULL-confidence form gives the first two outputs bit for bit."""
    H, W = shape
    planes = planted_planes(K, H, W, K, partition)
    (lab, score, lab2, score2, lse), clean = _merge(planes.cuda(), partition)
    rl, rs, rl2, rs2, rlse = stable_sort_reference(planes)
    assert clean
    assert torch.equal(lab, rl) and torch.equal(score, rs)
    assert torch.equal(lab2, rl2) and torch.equal(score2, rs2)
    d = (lse.double() - rlse).abs().max().item()
    print(f"lse vs fp64 logsumexp: max |d| = {d:.3e} (bound {lse_bound:.3e})")
    assert d <= lse_bound, (d, lse_bound)
    (lab_p, score_p, *rest), clean = _merge(planes.cuda(), partition, conf=False)
    assert clean and rest == [None, None, None]
    assert torch.equal(lab_p, lab) and torch.equal(score_p, score)


@pytest.mark.parametrize("off", [1, 2, 3])
def test_merge_labels_at_4_byte_aligned_offsets(off, lse_bound):
    """every buffer `off` elements into a 16-byte aligned allocation (and 9 x 261 planes, whose alignment moves from plane to plane): the
    16-byte runs start elsewhere, the values do not change and nothing outside the maps is written"""
    K, part = 37, [16, 16, 5]
    planes = planted_planes(K, 9, 261, K, part)
    (lab, score, lab2, score2, lse), clean = _merge(planes.cuda(), part, off=off)
    rl, rs, rl2, rs2, rlse = stable_sort_reference(planes)
    assert clean
    assert torch.equal(lab, rl) and torch.equal(score, rs) and torch.equal(lab2, rl2) and torch.equal(score2, rs2)
    assert (lse.double() - rlse).abs().max().item() <= lse_bound


def test_merge_labels_refuses_labels_beyond_int16():
    from lseg_hip import _lib
    lib = _lib.load()
    s = torch.zeros((2, 4, 4), device="cuda")
    lab = torch.zeros((4, 4), dtype=torch.int16, device="cuda")
    sc = torch.zeros((4, 4), device="cuda")
    assert lib.lseg_op_eval_merge_labels(_P(s), 2, 32766, 4, 4, _P(lab), _P(sc), None, None, None, 1, 1, _stream()) == ERR_UNSUPPORTED
    assert lib.lseg_op_eval_merge_labels(_P(s), 2, 32765, 4, 4, _P(lab), _P(sc), None, None, None, 1, 1, _stream()) == 0
    torch.cuda.synchronize()
    assert (lab == 32765).all()                                 # equal values: the lower label
    assert lib.lseg_op_eval_merge_labels(_P(s), 0, 0, 4, 4, _P(lab), _P(sc), None, None, None, 1, 1, _stream()) == ERR_INVALID
    assert lib.lseg_op_eval_merge_labels(_P(s), 2, 0, 4, 4, None, _P(sc), None, None, None, 1, 1, _stream()) == ERR_INVALID


# ---- the engine ------------------------------------------------------------------------------------------------------------------------
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


@pytest.mark.parametrize("image_dtype", ["bf16", None])
def test_score_features_is_forward_lowres_plane_for_plane(image_dtype):
    """K = 160 (the pixel_gram + generic GEMM route of forward_lowres): any slice of the label set scored from the held features is the
    matching planes of forward_lowres bit for bit -- the whole set (the 160-row label tile), panels of 64 / 64 / 32 and one row (64 x 64
    tiles): the tile the row count picks moves no bit."""
    warnings.simplefilter("ignore")
    from lseg_hip.synth import synthetic_images
    net = _net(image_dtype)
    x = synthetic_images(3, 64, 64, seed=7).cuda()
    with torch.no_grad():
        want = net.forward_lowres(x, MANY)
        assert want.shape == (3, 160, 32, 32)
        held = net.hold_features(x)
        assert held.B == 3 and held.size == (64, 64)
        out_c = net.cfg.out_c                                   # (128 on tiny16: the fused kernel's width is 512, so every K is on the generic route)
        assert held.feat.shape == (3, 18, 18, out_c) and held.feat.dtype == torch.float16 and held.scale.shape == (3, 32, 32)
        assert held.nbytes() == 3 * (18 * 18 * out_c * 2 + 32 * 32 * 4)
        for row0, rows in ((0, 160), (0, 64), (64, 64), (128, 32), (7, 1)):
            got = net.score_held(held, row0, rows, MANY)
            assert got.shape == (3, rows, 32, 32) and got.dtype == torch.float32
            assert torch.equal(got, want[:, row0:row0 + rows]), (row0, rows, (got - want[:, row0:row0 + rows]).abs().max().item())
        # the held features outlive other forwards of the engine
        net(x)
        assert torch.equal(net.score_held(held, 128, 32, MANY), want[:, 128:160])


@pytest.mark.parametrize("image_dtype", ["bf16", None])
def test_score_features_small_label_set_is_close_to_forward_lowres(image_dtype):
    """K = 5: where forward_lowres takes the fused kernel's cell dot products (out_c = 512, K <= 157) and the held features pixel_gram's,
    the last bits of the scale plane may differ.  Tolerance = 2 x the largest difference between forward_lowres by default and under
    LSEG_CORR_GENERIC=1 (the two existing routes, each in a fresh interpreter, the parent commit) on this input.  Measured: 0.0 with
    bf16 and with fp16 operands (|logit| up to 3.59): at tiny16's out_c = 128 both routes are the generic pair -- so the tolerance is
    0 and the planes must be equal."""
    warnings.simplefilter("ignore")
    from lseg_hip.synth import synthetic_images
    net = _net(image_dtype)
    x = synthetic_images(3, 64, 64, seed=7).cuda()
    tol = 2 * ROUTE_DIFF[image_dtype]
    with torch.no_grad():
        want = net.forward_lowres(x)
        held = net.hold_features(x)
        got = net.score_held(held, 0, 5)
        d = (got - want).abs().max().item()
        print(f"score_held vs forward_lowres, K = 5, {image_dtype or 'fp16'}: max |d| = {d:.3e} (tolerance {tol:.3e})")
        assert d <= tol, (d, tol)
        assert torch.equal(net.score_held(held, 1, 3), got[:, 1:4])          # a slice of our own route: bit for bit


def test_held_features_state_and_refusals():
    warnings.simplefilter("ignore")
    from lseg_hip import _lib
    from lseg_hip.synth import synthetic_images
    net = _net("bf16")                                          # the engine's train mode needs bf16 operands
    x = synthetic_images(3, 64, 64, seed=7).cuda()
    with torch.no_grad():
        net.forward_lowres(x)
        held = net.hold_features(x)
        eng = net._last_engine
        target = torch.zeros((3, 64, 64), dtype=torch.int64, device="cuda")
        with pytest.raises(_lib.LSegError) as e:                # the state of a streamed forward: no low-resolution logits exist
            eng.forward_stats(target)
        assert e.value.code == ERR_STATE
        with pytest.raises(_lib.LSegError) as e:
            eng.intermediate("lowres", (3, 5, 32, 32))
        assert e.value.code == ERR_STATE
        net.score_held(held, 0, 5)
        with pytest.raises(_lib.LSegError) as e:                # ... after score_features as well
            eng.forward_stats(target)
        assert e.value.code == ERR_STATE
        net.forward_lowres(x)                                   # another forward: the logits exist again
        eng.forward_stats(target)
        for row0, rows in ((0, 6), (5, 1), (3, 0), (-1, 2)):    # rows outside the 5 labels
            with pytest.raises(_lib.LSegError) as e:
                eng.score_features(held.feat, held.scale, row0, rows)
            assert e.value.code == ERR_INVALID, (row0, rows)
        # per-image label sets of either kind
        for kw in ({"labels_per_image": 1}, {"group_sizes": [1, 1, 1]}):
            eng.set_tokens(net.text[:3], **kw)
            with pytest.raises(_lib.LSegError) as e:
                eng.forward_features(x)
            assert e.value.code == ERR_UNSUPPORTED, kw
            with pytest.raises(_lib.LSegError) as e:
                eng.score_features(held.feat, held.scale, 0, 1)
            assert e.value.code == ERR_UNSUPPORTED, kw
        eng.set_tokens(net.text)
        eng._tok = None
        # train mode
        eng.set_train(True)
        try:
            with pytest.raises(_lib.LSegError) as e:
                eng.forward_features(x)
            assert e.value.code == ERR_UNSUPPORTED
            with pytest.raises(_lib.LSegError) as e:
                eng.score_features(held.feat, held.scale, 0, 1)
            assert e.value.code == ERR_UNSUPPORTED
        finally:
            eng.set_train(False)
        # the weights changed since hold_features
        net.scratch.head1.bias.add_(1.0)                        # (in place under no_grad: the tensor's version, hence the stamp, moves)
        with pytest.raises(RuntimeError, match="weights changed"):
            net.score_held(held, 0, 5)
    # head blocks: no commuted correlation
    net1 = _net(arch_option=1, block_depth=2)
    with torch.no_grad():
        with pytest.raises(_lib.LSegError) as e:
            net1.hold_features(x)
        assert e.value.code == ERR_UNSUPPORTED


# ---- the evaluator ---------------------------------------------------------------------------------------------------------------------
class _Mod(torch.nn.Module):
    def __init__(self, net, crop, base):
        super().__init__()
        self.net, self.crop_size, self.base_size = net, crop, base
        self.mean, self.std = [0.5] * 3, [0.5] * 3
        self._up_kwargs = {"mode": "bilinear", "align_corners": True}

    def evaluate_lowres(self, x):
        return self.net.forward_lowres(x)

    def evaluate_random_lowres(self, x, labelset):
        return self.net.forward_lowres(x, labelset)


class _HeldMod(_Mod):
    def hold_features(self, x):
        return self.net.hold_features(x)

    def score_held(self, held, row0, rows, labelset=""):
        return self.net.score_held(held, row0, rows, labelset)


SCALES = [0.5, 0.75, 1.0, 1.25, 1.5, 1.75]


@pytest.mark.parametrize("image_dtype", ["bf16", None])
def test_forward_labels_is_the_stable_sort_of_the_lowres_evaluator_scores(image_dtype, lse_bound):
    """80 x 104 image, crop 64, base 72, six scales + flip, max_batch 8, K = 160: forward_labels(confidence=True) at panel 160, 64 and 7,
    and windowed (max_stack 4), gives label / score / label2 / score2 equal to the stable sort of BatchedMultiEval(lowres=True).forward's
    scores bit for bit, hence identical across the panel sizes; lse within the op test's bound x K (the relative error of the K-term
    fp32 exp-sum grows at most linearly in K; 160 / 37 of it would be the tighter reading, the scores here reach two orders of magnitude
    beyond the op test's [-1, 1) and one fp32 step of such an lse alone is 7.6e-06); confidence=False gives the first two outputs."""
    warnings.simplefilter("ignore")
    from lseg_hip.evaluator import BatchedMultiEval
    from lseg_hip.synth import synthetic_images
    mod = _HeldMod(_net(image_dtype), crop=64, base=72)
    img = synthetic_images(1, 80, 104, seed=5).cuda()
    ev = BatchedMultiEval(mod, len(LABELS), flip=True, scales=SCALES, max_batch=8, lowres=True)
    with torch.no_grad():
        ref = ev(img, MANY)[0]
        assert ref.shape == (160, 80, 104)
        rl, rs, rl2, rs2, rlse = (t.cuda() for t in stable_sort_reference(ref.cpu()))
        first = None
        for panel, max_stack in ((160, None), (64, None), (7, None), (64, 4)):
            if max_stack is not None:
                ev.max_stack = max_stack
            lab, score, lab2, score2, lse = ev.forward_labels(img, MANY, confidence=True, panel=panel)
            assert lab.dtype == torch.int16 and lab.shape == score.shape == lab2.shape == score2.shape == lse.shape == (80, 104)
            assert torch.equal(lab, rl) and torch.equal(score, rs), (panel, max_stack)
            assert torch.equal(lab2, rl2) and torch.equal(score2, rs2), (panel, max_stack)
            d = (lse.double() - rlse).abs().max().item()
            print(f"panel {panel}, max_stack {max_stack}: lse vs fp64 logsumexp max |d| = {d:.3e} (bound {160 * lse_bound:.3e})")
            assert d <= 160 * lse_bound, (panel, d)
            if first is None:
                first = (lab, score, lab2, score2)
            assert all(torch.equal(a, b) for a, b in zip(first, (lab, score, lab2, score2)))
            if panel == 160:
                lab_p, score_p = ev.parallel_forward_labels([img[0]], MANY, panel=panel)[0]
                assert torch.equal(lab_p, lab) and torch.equal(score_p, score)
        del ev.max_stack


@pytest.mark.parametrize("image_dtype", ["bf16", None])
def test_forward_labels_with_the_modules_own_five_labels(image_dtype):
    """K = 5, the module's own labels, no pixel excluded: for every pixel ref_scores[our label] >= ref_best - t and |score - ref_best| <= t
    with t = 12 x the per-logit tolerance of the engine test (six scales x two twins enter a score, each count-normalised and
    interpolated with weights summing to one).  That tolerance was measured as 2 x 0.0 on this network (ROUTE_DIFF), so t = 0: the
    score is the reference's maximum exactly and our label attains it."""
    warnings.simplefilter("ignore")
    from lseg_hip.evaluator import BatchedMultiEval
    from lseg_hip.synth import synthetic_images
    mod = _HeldMod(_net(image_dtype), crop=64, base=72)
    img = synthetic_images(1, 80, 104, seed=5).cuda()
    ev = BatchedMultiEval(mod, len(LABELS), flip=True, scales=SCALES, max_batch=8, lowres=True)
    t = 12 * 2 * ROUTE_DIFF[image_dtype]
    with torch.no_grad():
        ref = ev(img)[0]
        lab, score = ev.forward_labels(img)
        best = ref.max(dim=0).values
        at_ours = ref.gather(0, lab.long().unsqueeze(0))[0]
        d_lab, d_score = (best - at_ours).max().item(), (score - best).abs().max().item()
        print(f"K = 5, {image_dtype or 'fp16'}: ref_best - ref[our label] max {d_lab:.3e}, |score - ref_best| max {d_score:.3e} (t = {t:.4f}); "
              f"{(lab.long() != ref.argmax(dim=0)).sum().item()} of {lab.numel()} labels differ")
        assert lab.min().item() >= 0 and lab.max().item() < 5
        assert d_lab <= t and d_score <= t, (d_lab, d_score, t)


def test_forward_labels_needs_hold_features_and_score_held():
    warnings.simplefilter("ignore")
    from lseg_hip.evaluator import BatchedMultiEval
    from lseg_hip.synth import synthetic_images
    ev = BatchedMultiEval(_Mod(_net(), crop=64, base=72), len(LABELS), flip=True, scales=SCALES, max_batch=8, lowres=True)
    with pytest.raises(AttributeError, match="hold_features"):
        ev.forward_labels(synthetic_images(1, 80, 104, seed=5).cuda())
