"""Label confidence without logits (lseg_forward_labels_conf / lseg_op_corr_argmax_conf, csrc/corr_argmax.hip CONF): the runner-up and
the log-sum-exp over the labels beside the arg-max -- against lseg_op_corr_argmax (bit-equal winner), against the label planes the
project's own plane kernels form (stable-sort top-2 bit-equal, lse within a measured bar), against an fp64 composition (large K), the
label-split workspace path, the guards, and the engine / network level on the streamed and the fallback routes.

The lse bar: 8 x the largest error fp32 torch.logsumexp itself shows against torch.logsumexp(planes.double(), 1) on the same planes.
On the MI355X the cases below printed (max |lse - fp64| of the kernel, of fp32 torch.logsumexp): see profiles/label_confidence.txt."""
import ctypes as C
import dataclasses
import functools
import os

import pytest
import torch
import torch.nn.functional as F

pytestmark = [pytest.mark.gpu, pytest.mark.gpu_fast]

from lseg_hip import _lib                                                        # noqa: E402
from lseg_hip.config import get_config                                           # noqa: E402
from lseg_hip.engine import HipEngine                                            # noqa: E402
from lseg_hip.synth import synthetic_state_dict, synthetic_tokens, synthetic_images   # noqa: E402

GUARD = 64
PLANES_MAX_K = 157                       # lseg_op_corr_planes holds T in LDS: K <= 157 per call


@pytest.fixture(scope="module")
def lib():
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    return _lib.load()


def P(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _op_case(B, K, H, W, seed):
    """tests/test_gpu_corr_argmax.py _op_case, rebuilt: fp16 g / T with a decisive winner almost everywhere (3 x 3 blocks of the base map
    carry the text row of one label each), 1e3 on the border of the padded map, and the LAST label a duplicate of the label of block
    (0, 0): wherever the original wins, the duplicate must be the runner-up with an identical score."""
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


class Guarded:
    """the five outputs with NaN / -7 guard bands around each"""
    NAMES = ("label", "score", "label2", "score2", "lse")

    def __init__(self, B, H, W, want=NAMES):
        self.n, self.shape = B * 16 * H * W, (B, 4 * H, 4 * W)
        self.buf = {k: (torch.full((self.n + 2 * GUARD,), -7, dtype=torch.int16) if k.startswith("label")
                        else torch.full((self.n + 2 * GUARD,), float("nan"))).cuda() for k in want}

    def ptr(self, k):
        return P(self.buf[k][GUARD:]) if k in self.buf else None

    def ptrs(self):
        return [self.ptr(k) for k in self.NAMES]

    def get(self, k):
        return self.buf[k][GUARD:GUARD + self.n].view(self.shape)

    def check_guards(self):
        for k, b in self.buf.items():
            ok = (lambda t: (t == -7).all()) if k.startswith("label") else (lambda t: torch.isnan(t).all())
            assert ok(b[:GUARD]) and ok(b[-GUARD:]), f"{k}: written outside the output"
            if not k.startswith("label"):
                assert not torch.isnan(self.get(k)).any(), f"{k}: an output pixel was not written"


def _conf(lib, g, T, scale, B, K, H, W, want=Guarded.NAMES, ws=None, ws_bytes=0):
    out = Guarded(B, H, W, want)
    _lib.check(lib.lseg_op_corr_argmax_conf(P(g), P(T), P(scale), *out.ptrs(), B, K, H, W, 512, P(ws), ws_bytes, stream()))
    torch.cuda.synchronize()
    out.check_guards()
    return out


def _planes(lib, g, T, scale, B, K, H, W):
    """the full-resolution logits of the project's own plane kernels: lseg_op_corr_planes (<= 157 labels per call: chunks of the text
    rows, a label's plane does not depend on its neighbours) + lseg_op_upsample4x_planes_scaled"""
    chunks = []
    for k0 in range(0, K, PLANES_MAX_K):
        kc = min(PLANES_MAX_K, K - k0)
        R = torch.zeros((B, kc, (H + 2) * (W + 2)), device="cuda")
        _lib.check(lib.lseg_op_corr_planes(P(g), P(T[k0:k0 + kc].contiguous()), P(R), None, B, kc, H, W, 512, stream()))
        chunks.append(R)
    R = torch.cat(chunks, 1).contiguous()
    out = torch.empty((B, K, 4 * H, 4 * W), device="cuda")
    _lib.check(lib.lseg_op_upsample4x_planes_scaled(P(R), P(scale), P(out), B, K, H, W, 0, None, stream()))
    torch.cuda.synchronize()
    return out


def _stable_top2(planes):
    s = torch.sort(planes, dim=1, descending=True, stable=True)
    return s.values[:, 0], s.indices[:, 0], s.values[:, 1], s.indices[:, 1]


def _lse_bar(planes):
    """(fp64 lse, 8 x the error of fp32 torch.logsumexp against it, that error)"""
    ref = torch.logsumexp(planes.double(), 1)
    own = (torch.logsumexp(planes, 1).double() - ref).abs().max().item()
    return ref, 8.0 * own, own


@functools.lru_cache(maxsize=None)
def _case(B, K, H, W, seed):
    """inputs, the plain arg-max, the full confidence run and the references of one case -- computed once, shared, never modified"""
    lib = _lib.load()
    g, T, scale, dup = _op_case(B, K, H, W, seed)
    n = B * 16 * H * W
    label0 = torch.full((B, 4 * H, 4 * W), -7, dtype=torch.int16).cuda()
    score0 = torch.full((B, 4 * H, 4 * W), float("nan")).cuda()
    _lib.check(lib.lseg_op_corr_argmax(P(g), P(T), P(scale), P(label0), P(score0), B, K, H, W, 512, None, 0, stream()))
    full = _conf(lib, g, T, scale, B, K, H, W)
    ref64 = _fp64_composition(g, T, scale, H, W)
    # the plane kernels need an even W; where they cannot form the planes the bar is measured the same way on the fp64 composition
    # rounded to fp32 (values of the same K and magnitude: what the bar depends on)
    planes = _planes(lib, g, T, scale, B, K, H, W) if W % 2 == 0 else None
    lse64, bar, own = _lse_bar(planes if planes is not None else ref64.float())
    return dict(g=g, T=T, scale=scale, dup=dup, n=n, label0=label0, score0=score0, full=full, planes=planes, ref64=ref64,
                lse64=lse64 if planes is not None else None, bar=bar, own=own)


# (B, K, H, W, seed): the shapes of the issue with the seeds tests/test_gpu_corr_argmax.py uses for them, + one more that the plane
# kernels can form (even W) with several tiles, four panels and a ragged last one
CASES = [(1, 16, 6, 6, 1), (2, 157, 15, 15, 2), (1, 158, 30, 30, 3), (2, 300, 9, 17, 4), (1, 1000, 6, 6, 7), (2, 157, 16, 14, 8)]
EXACT_CASES = [cs for cs in CASES if cs[3] % 2 == 0]        # K > 157: the planes are formed in chunks of the text rows


@pytest.mark.parametrize("B,K,H,W,seed", CASES)
def test_winner_is_bit_equal_to_corr_argmax_with_any_subset_of_outputs_and_with_the_label_split(lib, B, K, H, W, seed):
    c = _case(B, K, H, W, seed)
    full = c["full"]
    assert torch.equal(full.get("label"), c["label0"]) and torch.equal(full.get("score"), c["score0"])
    assert (full.get("label2") >= 0).all() and (full.get("label2") < K).all() and (full.get("label2") != full.get("label")).all()
    assert torch.isfinite(full.get("score2")).all() and (full.get("score2") <= full.get("score")).all()
    assert (full.get("lse") >= full.get("score")).all()
    # the duplicated last label: wherever the original wins, the duplicate is the runner-up with an identical score
    won = full.get("label") == c["dup"]
    assert won.any() and (full.get("label2")[won] == K - 1).all() and torch.equal(full.get("score2")[won], full.get("score")[won])
    # fewer optional outputs: the ones asked for are the same bits
    for want in (("label", "label2"), ("label", "lse"), ("label", "score2"), ("label", "score", "score2", "lse"), ("label", "score")):
        part = _conf(lib, c["g"], c["T"], c["scale"], B, K, H, W, want)
        for k in want:
            assert torch.equal(part.get(k), full.get(k)), (want, k)
    # the label split: room for 8 parts of 16 bytes per output pixel; top-2 by the same rule, lse in another summation order
    ws = torch.empty((8 * c["n"] * 16 + 4 * GUARD,), dtype=torch.uint8).cuda()
    split = _conf(lib, c["g"], c["T"], c["scale"], B, K, H, W, ws=ws, ws_bytes=8 * c["n"] * 16)
    for k in ("label", "score", "label2", "score2"):
        assert torch.equal(split.get(k), full.get(k)), k
    d = (split.get("lse").double() - full.get("lse").double()).abs().max().item()
    print(f"conf op B={B} K={K} {H}x{W}: max|lse(split) - lse| {d:.3e}, bar {c['bar']:.3e} (fp32 torch.logsumexp vs fp64: {c['own']:.3e})")
    assert d <= c["bar"]


@pytest.mark.parametrize("B,K,H,W,seed", EXACT_CASES)
def test_top2_is_the_stable_sort_of_the_planes_and_lse_meets_the_measured_bar(lib, B, K, H, W, seed):
    """Of the issue's shapes with K <= 157 only 6 x 6 has the even W lseg_op_upsample4x_planes_scaled needs (15 x 15 does not): the
    16 x 14 case stands in for it, and the K = 158 / 1000 shapes are compared too, their planes formed 157 text rows at a time."""
    c = _case(B, K, H, W, seed)
    full = c["full"]
    v0, i0, v1, i1 = _stable_top2(c["planes"])
    assert torch.equal(full.get("label").long(), i0) and torch.equal(full.get("score"), v0)
    assert torch.equal(full.get("label2").long(), i1) and torch.equal(full.get("score2"), v1)
    err = (full.get("lse").double() - c["lse64"]).abs().max().item()
    print(f"conf op B={B} K={K} {H}x{W}: max|lse - fp64 logsumexp(planes)| {err:.3e}; fp32 torch.logsumexp {c['own']:.3e}; bar {c['bar']:.3e}")
    assert err <= c["bar"]


def _fp64_composition(g, T, scale, H, W):
    R = torch.einsum("kc,byxc->bkyx", T.double(), g[:, 1:H + 1, 1:W + 1].double())
    mid = F.interpolate(R, scale_factor=2, mode="bilinear", align_corners=True) * scale.double().unsqueeze(1)
    return F.interpolate(mid, scale_factor=2, mode="bilinear", align_corners=True)


def fp64_conditions(ref, label, score, label2, score2, lse):
    """the issue's conditions against an fp64 composition; runner-up labels are judged by value, so near-ties need no exclusions"""
    amax = ref.abs().max().item()
    tol = 2e-3 * amax
    top2 = ref.topk(2, dim=1).values
    ref_second = top2[:, 1]
    own2 = ref.gather(1, label2.long().unsqueeze(1)).squeeze(1)
    lse64 = torch.logsumexp(ref, 1)
    figures = dict(score=(score.double() - top2[:, 0]).abs().max().item(), score2=(score2.double() - ref_second).abs().max().item(),
                   label2=(ref_second - own2).max().item(), lse=(lse.double() - lse64).abs().max().item(), tol=tol)
    print("fp64 composition:", ", ".join(f"{k} {v:.3e}" for k, v in figures.items()))
    assert (label2 != label).all()
    assert figures["score2"] <= tol
    assert (own2 >= ref_second - 2 * tol).all()
    assert figures["lse"] <= tol + 1e-4
    return figures


@pytest.mark.parametrize("B,K,H,W,seed", CASES)            # K = 300 / 1000 have no other value reference; the rest come along
def test_against_the_fp64_composition(lib, B, K, H, W, seed):
    c = _case(B, K, H, W, seed)
    full = c["full"]
    fp64_conditions(c["ref64"], full.get("label"), full.get("score"), full.get("label2"), full.get("score2"), full.get("lse"))


def test_guards_and_the_single_label(lib):
    g = (0.1 * torch.randn((1, 6, 6, 512), generator=torch.Generator().manual_seed(0))).half().cuda()
    T = torch.zeros((40000, 512), dtype=torch.float16)
    T[0] = F.normalize(torch.randn(512, generator=torch.Generator().manual_seed(1)), dim=0).half()
    T = T.cuda()
    sc = torch.full((1, 8, 8), 10.0).cuda()
    o = Guarded(1, 4, 4)
    call = lib.lseg_op_corr_argmax_conf
    assert call(P(g), P(T), P(sc), *o.ptrs(), 1, 40000, 4, 4, 512, None, 0, stream()) == -5          # K > 32767: LSEG_ERR_UNSUPPORTED
    assert b"32767" in lib.lseg_last_error(None)
    assert call(P(g), P(T), P(sc), *o.ptrs(), 1, 8, 4, 4, 768, None, 0, stream()) == -5              # other widths
    assert call(P(g), P(T), P(sc), None, *o.ptrs()[1:], 1, 8, 4, 4, 512, None, 0, stream()) == -1    # NULL label output: LSEG_ERR_INVALID
    assert call(None, P(T), P(sc), *o.ptrs(), 1, 8, 4, 4, 512, None, 0, stream()) == -1
    assert call(P(g), None, P(sc), *o.ptrs(), 1, 8, 4, 4, 512, None, 0, stream()) == -1
    assert call(P(g), P(T), None, *o.ptrs(), 1, 8, 4, 4, 512, None, 0, stream()) == -1
    torch.cuda.synchronize()
    assert all(torch.isnan(o.get(k)).all() for k in ("score", "score2", "lse")), "a refused call wrote an output"
    # K = 1: no runner-up -- label2 = -1, score2 = -inf, lse = score (documented in include/lseg_hip.h)
    _lib.check(call(P(g), P(T), P(sc), *o.ptrs(), 1, 1, 4, 4, 512, None, 0, stream()))
    torch.cuda.synchronize()
    o.check_guards()
    assert (o.get("label") == 0).all() and (o.get("label2") == -1).all()
    assert torch.isinf(o.get("score2")).all() and (o.get("score2") < 0).all()
    assert torch.isfinite(o.get("score")).all() and torch.equal(o.get("lse"), o.get("score"))


# ---- engine / network level ----------------------------------------------------------------------------------------------------------
def _check_against_own_logits(eng, x, K):
    """forward_labels_conf against the engine's own forward() logits: stable-sort top-2 bit-equal, lse inside the measured bar; the
    winner equal to forward_labels.  Returns the confidence dict and the logits."""
    r = eng.forward_labels_conf(x)
    lab, score = eng.forward_labels(x, want_score=True)
    out = eng.forward(x)
    torch.cuda.synchronize()
    assert r["label"].dtype == torch.int16 and r["label2"].dtype == torch.int16 and all(v.shape == lab.shape for v in r.values())
    assert torch.equal(r["label"], lab) and torch.equal(r["score"], score)
    v0, i0, v1, i1 = _stable_top2(out)
    assert torch.equal(r["label"].long(), i0) and torch.equal(r["score"], v0)
    assert torch.equal(r["label2"].long(), i1) and torch.equal(r["score2"], v1)
    ref, bar, own = _lse_bar(out)
    err = (r["lse"].double() - ref).abs().max().item()
    print(f"engine K={K}: max|lse - fp64 logsumexp(logits)| {err:.3e}; fp32 torch.logsumexp {own:.3e}; bar {bar:.3e}")
    assert err <= bar
    return r, out


def test_engine_streamed_vitl16_k120():
    """ViT-L/16, out_c 512, arch_option 0, one shared set of 120 labels at 96 x 96: streamed (three panels, split over label parts in the
    engine's workspace).  After it no low-resolution logits exist, as after forward_labels."""
    K = 120
    cfg = get_config("clip_vitl16_384", arch_option=0, block_depth=0, activation="lrelu")
    eng = HipEngine(cfg, 96, 96, max_batch=2, max_labels=K, image_dtype="fp16")
    eng.load_state_dict(synthetic_state_dict(cfg, seed=11))
    eng.set_tokens(synthetic_tokens([f"thing {i}" for i in range(K)], cfg.text.vocab, cfg.text.ctx))
    x = synthetic_images(2, 96, 96, seed=11).cuda()
    eng.forward_labels_conf(x)
    with pytest.raises(_lib.LSegError) as e:
        eng.forward_stats(torch.zeros((2, 96, 96), dtype=torch.long).cuda())
    assert e.value.code == -4 and "labels-only" in str(e.value)                          # streamed: LSEG_ERR_STATE
    _check_against_own_logits(eng, x, K)
    eng.close()


def test_engine_fallback_head_blocks(golden_dir):
    """arch_option 1 (head blocks) cannot stream: the reduction runs on the planes in memory, which stay there."""
    g = torch.load(os.path.join(golden_dir, "ref_vitl16_96x96_k5_arch1.pt"))
    bb, H, W, B, K, seed, arch, depth = g["spec"]
    cfg = get_config(bb, arch_option=arch, block_depth=depth, activation="lrelu")
    eng = HipEngine(cfg, H, W, max_batch=B, max_labels=K, image_dtype="fp16")
    eng.load_state_dict(synthetic_state_dict(cfg, seed=seed))
    eng.set_tokens(g["tokens"])
    x = synthetic_images(B, H, W, seed=seed).cuda()
    eng.forward_labels_conf(x)
    r = eng.forward_stats(torch.zeros((B, H, W), dtype=torch.long).cuda())               # the planes exist
    assert int(r["labeled"]) == B * H * W
    _check_against_own_logits(eng, x, K)
    eng.close()


def test_engine_fallback_per_image_label_sets_of_two():
    """3 images x 2 labels each: the runner-up is the other label and exp(score - lse) is the 2-class softmax of the engine's own logits."""
    cfg = get_config("tiny16")
    eng = HipEngine(cfg, 64, 64, max_batch=3, max_labels=6, image_dtype="fp16")
    eng.load_state_dict(synthetic_state_dict(cfg, seed=5))
    eng.set_tokens(synthetic_tokens(["cat", "other", "sky", "other", "tree", "other"], cfg.text.vocab, cfg.text.ctx), labels_per_image=2)
    x = synthetic_images(3, 64, 64, seed=5).cuda()
    r, out = _check_against_own_logits(eng, x, 2)
    assert out.shape == (3, 2, 64, 64)
    assert torch.equal(r["label2"], 1 - r["label"])
    prob = torch.exp(r["score"] - r["lse"]).double()
    ref = torch.softmax(out.double(), 1).max(1).values
    # |d prob| <= prob * |d(score - lse)|: the lse bar of this case (8 x fp32 logsumexp's own error) + the rounding of the fp32 exp
    _, bar, _ = _lse_bar(out)
    assert (prob - ref).abs().max().item() <= bar + 4 * 2.0 ** -24
    eng.close()


def test_engine_single_label_per_image_has_no_runner_up():
    cfg = get_config("tiny16")
    eng = HipEngine(cfg, 64, 64, max_batch=2, max_labels=2, image_dtype="fp16")
    eng.load_state_dict(synthetic_state_dict(cfg, seed=5))
    eng.set_tokens(synthetic_tokens(["cat", "sky"], cfg.text.vocab, cfg.text.ctx), labels_per_image=1)
    r = eng.forward_labels_conf(synthetic_images(2, 64, 64, seed=5).cuda())
    torch.cuda.synchronize()
    assert (r["label"] == 0).all() and (r["label2"] == -1).all() and torch.isinf(r["score2"]).all() and (r["score2"] < 0).all()
    assert torch.equal(r["lse"], r["score"])
    eng.close()


def test_engine_entry_null_pointers_and_a_single_optional_output():
    cfg = get_config("tiny16")
    eng = HipEngine(cfg, 64, 64, max_batch=1, max_labels=3, image_dtype="fp16")
    eng.load_state_dict(synthetic_state_dict(cfg, seed=0))
    eng.set_tokens(synthetic_tokens(["a", "b", "c"], cfg.text.vocab, cfg.text.ctx))
    x = synthetic_images(1, 64, 64, seed=0).cuda()
    lab = torch.empty((1, 64, 64), dtype=torch.int16).cuda()
    lse = torch.empty((1, 64, 64)).cuda()
    call = eng.lib.lseg_forward_labels_conf
    assert call(eng._h, P(x), 1, None, None, None, None, P(lse), stream()) == -1         # NULL label output
    assert call(eng._h, None, 1, P(lab), None, None, None, P(lse), stream()) == -1       # NULL input
    _lib.check(call(eng._h, P(x), 1, P(lab), None, None, None, P(lse), stream()))        # only lse beside the label
    torch.cuda.synchronize()
    assert torch.equal(lab, eng.forward_labels(x)) and torch.equal(lse, eng.forward_labels_conf(x)["lse"])
    eng.close()


def test_predict_labels_with_confidence():
    """LSegNet.predict_labels(confidence=True): prob in (0, 1], margin >= 0, and the default call returns what it returned before."""
    from modules.models.lseg_net import LSegNet
    labels = [f"thing {i}" for i in range(300)]
    cfg = get_config("tiny16")
    net = LSegNet(labels=labels, backbone="tiny16", features=cfg.features, arch_option=0, block_depth=0, activation="lrelu")
    net.load_state_dict(synthetic_state_dict(cfg, seed=0))
    net = net.eval().cuda()
    x = synthetic_images(2, 64, 64, seed=0).cuda()
    with torch.no_grad():
        out = net(x)
    plain = net.predict_labels(x)
    r = net.predict_labels(x, confidence=True)
    assert isinstance(plain, torch.Tensor) and plain.dtype == torch.long and plain.shape == (2, 64, 64)
    assert torch.equal(plain, net._last_engine.forward_labels(x).long())                 # the default: exactly the forward_labels mask
    assert set(r) == {"label", "prob", "label2", "margin"}
    assert torch.equal(r["label"], plain) and r["label2"].dtype == torch.long
    assert (r["prob"] > 0).all() and (r["prob"] <= 1).all() and (r["margin"] >= 0).all()
    v0, i0, v1, i1 = _stable_top2(out)
    assert torch.equal(r["label"], i0) and torch.equal(r["label2"], i1) and torch.equal(r["margin"], v0 - v1)
    ref = torch.softmax(out.double(), 1).max(1).values
    _, bar, _ = _lse_bar(out)
    assert (r["prob"].double() - ref).abs().max().item() <= bar + 4 * 2.0 ** -24
