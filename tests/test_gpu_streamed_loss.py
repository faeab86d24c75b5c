"""Cross-entropy on the streamed label route (lseg_op_corr_argmax_loss / lseg_forward_labels_loss, csrc/corr_argmax.hip LOSS): the target's
logit kept while its label passes through the registers, the online log-sum-exp of the CONF instantiation, a fixed-order reduction.

Operator: B = 2, quarter-resolution maps 6 x 6 (even W: the project's plane kernels form exact planes) and 15 x 15 (tile edges), K in
{1, 5, 48, 49, 157, 300} -- the panel of 48 on both sides, a last partial panel, beyond the planes kernel's 157 -- unsplit and with a
workspace for 8 label parts, ragged lists of [1, 49, 5] labels.  Every target holds a row of ignore_index, of values >= K, of a negative
value that is not ignore_index, of the winner's own label, of label 0 and of label K - 1 (streamed_loss_helpers.make_target).
Bars: lse as tests/test_gpu_label_confidence.py measures it (8 x fp32 torch.logsumexp's own error against fp64 on the same planes);
against the fp64 composition the per-pixel |nll - CE64| is bounded by the score bar plus the lse bar of that file's fp64_conditions
(2e-3 max|ref| and 2e-3 max|ref| + 1e-4).

Engine: the synthetic small network widened to out_c = 512 (streamed, as tests/test_gpu_ragged_labels.py does) for the shared set and
the per-image lists; head blocks (arch_option 1) as the fallback configuration.  Per-image lists: the issue's alternative is taken --
image b of the ragged run is compared with a shared-set run of list b and target b -- in the SAME batch rather than at B = 1, so that
the image tower is bit-identical and the comparison is exact for label / score / counts and inside the lse bar for the loss."""
import ctypes as C
import dataclasses
import functools
import os

import pytest
import torch
import torch.nn.functional as F

pytestmark = [pytest.mark.gpu, pytest.mark.gpu_fast]

from lseg_hip import _lib                                                        # noqa: E402
from lseg_hip import config as lseg_config                                       # noqa: E402
from lseg_hip.config import get_config                                           # noqa: E402
from lseg_hip.engine import HipEngine                                            # noqa: E402
from lseg_hip.synth import synthetic_state_dict, synthetic_tokens, synthetic_images   # noqa: E402
from streamed_loss_helpers import GUARD, LossOutputs, make_target, valid_mask    # noqa: E402
from test_gpu_label_confidence import P, stream, _op_case, _planes, _lse_bar, _fp64_composition   # noqa: E402

B = 2
KS = (1, 5, 48, 49, 157, 300)
SIZES = (6, 15)
CASES = [(K, S) for S in SIZES for K in KS]


@pytest.fixture(scope="module")
def lib():
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    return _lib.load()


def _ign(K):
    return 255 if K < 200 else -1            # a non-negative ignore_index (a label id when K > 255 would allow it: there -1)


def _inputs(Bn, K, H, W, seed):
    """the builders of tests/test_gpu_label_confidence.py; they need K >= 2 (the last label is a duplicate): K = 1 takes row 0 of K = 2"""
    g, T, scale, _ = _op_case(Bn, max(K, 2), H, W, seed)
    return g, T[:K].contiguous(), scale


def _run(lib, g, T, scale, target, ign, Bn, K, H, W, want=LossOutputs.NAMES, parts=0, counts=None):
    out = LossOutputs(Bn, H, W, want)
    red = "nll" in want or "nll_plane" in want
    temps = (("lse" not in want) + ("tlogit" not in want)) if red else 0
    nbytes = lib.lseg_op_corr_argmax_loss_ws_bytes(Bn, H, W, int(counts is not None), int("nll" in want), temps, parts)
    ws = torch.empty((nbytes + 2 * GUARD,), dtype=torch.uint8).cuda() if nbytes else None
    hc = (C.c_int32 * Bn)(*counts) if counts is not None else None
    _lib.check(lib.lseg_op_corr_argmax_loss(P(g), P(T), P(scale), P(target), ign, hc, Bn, K, H, W, 512, *out.ptrs(), P(ws), nbytes, stream()))
    torch.cuda.synchronize()
    out.check_guards()
    return out


def _would_split(lib, Bn, K, H, W):
    """the label parts the launcher takes for this shape with room for 8 (the split depends on panels, tiles and compute units only)"""
    out2 = (C.c_int * 2)()
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    _lib.check(lib.lseg_op_corr_argmax_ragged_split((C.c_int32 * Bn)(*([K] * Bn)), Bn, H, W, 1, 8 * Bn * 16 * H * W * 16, cus, out2))
    return out2[0]


@functools.lru_cache(maxsize=None)
def _case(K, S):
    """inputs, target, the references and the unsplit / split runs of one case: computed once, shared, never modified"""
    lib = _lib.load()
    H = W = S
    g, T, scale = _inputs(B, K, H, W, 100 + K + S)
    label0 = torch.full((B, 4 * H, 4 * W), -7, dtype=torch.int16).cuda()
    score0 = torch.full((B, 4 * H, 4 * W), float("nan")).cuda()
    _lib.check(lib.lseg_op_corr_argmax(P(g), P(T), P(scale), P(label0), P(score0), B, K, H, W, 512, None, 0, stream()))
    lse0 = torch.full((B, 4 * H, 4 * W), float("nan")).cuda()
    lab1 = torch.empty_like(label0)
    _lib.check(lib.lseg_op_corr_argmax_conf(P(g), P(T), P(scale), P(lab1), None, None, None, P(lse0), B, K, H, W, 512, None, 0, stream()))
    torch.cuda.synchronize()
    ign = _ign(K)
    target = make_target(label0, K, ign, seed=K + S).cuda()
    valid = torch.from_numpy(valid_mask(target.cpu().numpy(), ign, K)).cuda()
    full = _run(lib, g, T, scale, target, ign, B, K, H, W)
    split = _run(lib, g, T, scale, target, ign, B, K, H, W, parts=8)
    ref64 = _fp64_composition(g, T, scale, H, W)
    planes = _planes(lib, g, T, scale, B, K, H, W) if W % 2 == 0 else None
    lse64, bar, own = _lse_bar(planes if planes is not None else ref64.float())
    return dict(g=g, T=T, scale=scale, ign=ign, target=target, valid=valid, label0=label0, score0=score0, lse0=lse0, full=full, split=split,
                ref64=ref64, planes=planes, lse64=lse64 if planes is not None else None, bar=bar, own=own, nsplit=_would_split(lib, B, K, H, W))


@pytest.mark.parametrize("K,S", CASES)
def test_winner_target_logit_and_invalid_pixels(lib, K, S):
    c = _case(K, S)
    full, t, valid = c["full"], c["target"], c["valid"]
    # 1. the winner is lseg_op_corr_argmax's, bit for bit (and the sum is the CONF instantiation's)
    assert torch.equal(full.get("label"), c["label0"]) and torch.equal(full.get("score"), c["score0"])
    assert torch.equal(full.get("lse"), c["lse0"])
    # the target rows are what they claim to be
    assert (t[:, 0] == c["ign"]).all() and (t[:, 1] >= K).all() and (t[:, 2] < 0).all() and (t[:, 2] != c["ign"]).all()
    assert torch.equal(t[:, 3], c["label0"][:, 3].long()) and (t[:, 4] == 0).all() and (t[:, 5] == K - 1).all()
    assert not valid[:, :3].any() and valid[:, 3:6].all()
    # 2. where the target is the winner, its logit is the score
    hit = valid & (t == full.get("label").long())
    assert hit[:, 3].all() and torch.equal(full.get("tlogit")[hit], full.get("score")[hit])
    # 3. invalid pixels: tlogit = -inf, plane = 0, not counted; valid pixels: finite, plane = lse - tlogit >= 0
    tl, plane = full.get("tlogit"), full.get("nll_plane")
    assert torch.isinf(tl[~valid]).all() and (tl[~valid] < 0).all() and (plane[~valid] == 0).all()
    assert torch.isfinite(tl[valid]).all() and (tl[valid] <= full.get("score")[valid]).all()
    assert torch.equal(plane[valid], (full.get("lse") - tl)[valid]) and (plane >= 0).all()
    # 7. the count
    nll = full.get("nll").cpu()
    nv = int(valid.sum())
    assert nll[1].item() == nv and nv > 0
    # 8. the sum against the planes it was formed from: every term >= 0, so a reordered double sum differs by <= n * 2^-52 relative
    ref = (full.get("lse").double() - tl.double())[valid].sum().item()
    print(f"loss op K={K} {S}x{S}: nll {nll[0].item():.9e} / {nv} valid; |sum - torch sum| {abs(nll[0].item() - ref):.3e}")
    assert abs(nll[0].item() - ref) <= nv * 2.0 ** -52 * abs(ref)
    # K = 1: lse == score, and the loss is exactly 0 where the target is label 0
    if K == 1:
        assert torch.equal(full.get("lse"), full.get("score")) and (plane == 0).all() and nll[0].item() == 0.0


@pytest.mark.parametrize("K,S", CASES)
def test_two_runs_and_any_subset_of_outputs_give_the_same_bits(lib, K, S):
    c = _case(K, S)
    full = c["full"]
    again = _run(lib, c["g"], c["T"], c["scale"], c["target"], c["ign"], B, K, S, S)
    for k in LossOutputs.NAMES:                                                   # 9. (nll among them) bit-identical
        assert torch.equal(again.get(k), full.get(k)), k
    for want in (("label",), ("label", "nll"), ("label", "nll_plane"), ("label", "tlogit"), ("label", "lse", "nll"), ("label", "score", "tlogit", "nll")):
        part = _run(lib, c["g"], c["T"], c["scale"], c["target"], c["ign"], B, K, S, S, want)
        for k in want:
            assert torch.equal(part.get(k), full.get(k)), (want, k)


@pytest.mark.parametrize("K,S", CASES)
def test_label_split_equals_the_unsplit_form(lib, K, S):
    c = _case(K, S)
    full, split = c["full"], c["split"]
    assert (c["nsplit"] > 1) == (K > 48), "a label set of more than one panel must take the split here"
    for k in ("label", "score", "tlogit"):                                        # 10.
        assert torch.equal(split.get(k), full.get(k)), k
    d = (split.get("lse").double() - full.get("lse").double()).abs().max().item()
    print(f"loss op K={K} {S}x{S}: {c['nsplit']} parts, max|lse(split) - lse| {d:.3e}, bar {c['bar']:.3e}")
    assert d <= c["bar"]
    assert split.get("nll")[1].item() == full.get("nll")[1].item()
    nv = int(c["valid"].sum())
    assert abs(split.get("nll")[0].item() - full.get("nll")[0].item()) <= nv * c["bar"]
    if c["nsplit"] == 1:
        assert torch.equal(split.get("lse"), full.get("lse")) and torch.equal(split.get("nll"), full.get("nll"))


@pytest.mark.parametrize("K", KS)
def test_target_logit_is_the_plane_value_and_lse_meets_the_measured_bar(lib, K):
    """6 x 6 only (lseg_op_upsample4x_planes_scaled needs an even W); K = 300: the planes are formed 157 text rows at a time"""
    c = _case(K, 6)
    full, valid = c["full"], c["valid"]
    own = c["planes"].gather(1, c["target"].clamp(0, K - 1).unsqueeze(1)).squeeze(1)
    assert torch.equal(full.get("tlogit")[valid], own[valid])                     # 4.
    err = (full.get("lse").double() - c["lse64"]).abs().max().item()              # 5.
    print(f"loss op K={K} 6x6: max|lse - fp64 logsumexp(planes)| {err:.3e}; fp32 torch.logsumexp {c['own']:.3e}; bar {c['bar']:.3e}")
    assert err <= c["bar"]
    for name in ("split",):
        err = (c[name].get("lse").double() - c["lse64"]).abs().max().item()
        assert err <= c["bar"], (name, err)


@pytest.mark.parametrize("K,S", CASES)
def test_against_the_fp64_composition(lib, K, S):
    c = _case(K, S)
    ref, valid, t = c["ref64"], c["valid"], c["target"]
    tol = 2e-3 * ref.abs().max().item()                                           # fp64_conditions: the score bar; its lse bar is tol + 1e-4
    ce64 = torch.logsumexp(ref, 1) - ref.gather(1, t.clamp(0, K - 1).unsqueeze(1)).squeeze(1)
    for name in ("full", "split"):
        plane = c[name].get("nll_plane").double()
        d = (plane - ce64).abs()[valid].max().item()
        print(f"loss op K={K} {S}x{S} {name}: max|nll - CE64| {d:.3e}, bound {2 * tol + 1e-4:.3e}")
        assert d <= 2 * tol + 1e-4                                                # 6.


RAGGED = [1, 49, 5]


@pytest.mark.parametrize("S", SIZES)
@pytest.mark.parametrize("parts", (0, 8))
def test_ragged_image_equals_the_shared_set_run_on_its_slices(lib, S, parts):
    """11. image b of the ragged call == the shared-set call with B = 1, list b and target b (with a workspace: lse inside the bar)"""
    Bn, H, W = len(RAGGED), S, S
    g, T, scale = _inputs(Bn, sum(RAGGED), H, W, 7 + S)
    ign = -100
    label0 = torch.zeros((Bn, 4 * H, 4 * W), dtype=torch.int16)
    target = torch.cat([make_target(label0[b:b + 1], k, ign, seed=b) for b, k in enumerate(RAGGED)]).cuda()
    target[1, 3] = 48                                                             # (no winner known yet: the last label instead)
    r = _run(lib, g, T, scale, target, ign, Bn, 0, H, W, parts=parts, counts=RAGGED)
    valid = torch.from_numpy(valid_mask(target.cpu().numpy(), ign, RAGGED)).cuda()
    assert r.get("nll")[1].item() == int(valid.sum())
    total, r0 = 0.0, 0
    for b, k in enumerate(RAGGED):
        one = _run(lib, g[b:b + 1].contiguous(), T[r0:r0 + k].contiguous(), scale[b:b + 1].contiguous(), target[b:b + 1].contiguous(), ign,
                   1, k, H, W)
        r0 += k
        for name in ("label", "score", "tlogit"):
            assert torch.equal(r.get(name)[b], one.get(name)[0]), (b, name)
        assert (r.get("label")[b] < k).all()
        if parts == 0:
            assert torch.equal(r.get("lse")[b], one.get("lse")[0]) and torch.equal(r.get("nll_plane")[b], one.get("nll_plane")[0])
        else:
            ref64 = _fp64_composition(g[b:b + 1], T[r0 - k:r0], scale[b:b + 1], H, W)
            _, bar, _ = _lse_bar(ref64.float())
            assert (r.get("lse")[b].double() - one.get("lse")[0].double()).abs().max().item() <= bar
        assert (r.get("nll_plane")[b][~valid[b]] == 0).all() and torch.isinf(r.get("tlogit")[b][~valid[b]]).all()
        total += one.get("nll")[0].item()
    if parts == 0:
        nv = int(valid.sum())
        assert abs(r.get("nll")[0].item() - total) <= nv * 2.0 ** -52 * abs(total)


def test_guards_refuse_before_anything_is_launched(lib):
    """12. refused calls return before a launch and leave the guard-banded outputs untouched"""
    H = W = 6
    g, T, scale = _inputs(1, 8, H, W, 3)
    Tbig = torch.zeros((40000, 512), dtype=torch.float16).cuda()
    target = torch.zeros((1, 24, 24), dtype=torch.int64).cuda()
    o = LossOutputs(1, H, W)
    nbytes = lib.lseg_op_corr_argmax_loss_ws_bytes(1, H, W, 1, 1, 0, 0)
    ws = torch.empty((nbytes,), dtype=torch.uint8).cuda()
    call = lib.lseg_op_corr_argmax_loss
    tail = (P(ws), nbytes, stream())
    assert call(P(g), P(Tbig), P(scale), P(target), -1, None, 1, 40000, H, W, 512, *o.ptrs(), *tail) == -5      # K > 32767
    assert b"32767" in lib.lseg_last_error(None)
    assert call(P(g), P(T), P(scale), P(target), -1, None, 1, 8, H, W, 768, *o.ptrs(), *tail) == -5             # other widths
    assert call(P(g), P(T), P(scale), P(target), -1, None, 1, 8, H, W, 512, None, *o.ptrs()[1:], *tail) == -1   # NULL label output
    assert call(P(g), P(T), P(scale), None, -1, None, 1, 8, H, W, 512, *o.ptrs(), *tail) == -1                  # NULL target
    assert call(None, P(T), P(scale), P(target), -1, None, 1, 8, H, W, 512, *o.ptrs(), *tail) == -1
    assert call(P(g), None, P(scale), P(target), -1, None, 1, 8, H, W, 512, *o.ptrs(), *tail) == -1
    assert call(P(g), P(T), None, P(target), -1, None, 1, 8, H, W, 512, *o.ptrs(), *tail) == -1
    assert call(P(g), P(T), P(scale), P(target), -1, None, 1, 8, H, W, 512, *o.ptrs(), None, 0, stream()) == -1  # the sum needs its partials
    assert b"workspace" in lib.lseg_last_error(None)
    assert call(P(g), P(T), P(scale), P(target), -1, (C.c_int32 * 1)(0), 1, 8, H, W, 512, *o.ptrs(), *tail) == -1   # an empty list
    assert call(P(g), P(T), P(scale), P(target), -1, (C.c_int32 * 1)(8), 1, 8, H, W, 512, *o.ptrs(), None, 0, stream()) == -1   # ragged: offsets
    torch.cuda.synchronize()
    assert o.untouched(), "a refused call wrote an output"


def _same_bits_across_the_modes(argmax, conf, loss):
    """(label, score) of the arg-max, the confidence and the loss form, lse of the last two: the three modes share their per-value code,
    so they agree bit for bit.  No pixel may tie in its top two (score > score2), so an equal label cannot hide behind the tie order"""
    assert (conf["score"] > conf["score2"]).all(), "a tie in the top two: pick another seed"
    for k in ("label", "score"):
        assert torch.equal(argmax[k], conf[k]) and torch.equal(loss[k], conf[k]), k
    assert torch.equal(loss["lse"], conf["lse"])


def test_the_three_modes_agree_bit_for_bit_on_split_labels(lib):
    """B = 2, 15 x 15 (30 mid rows: two tiles per axis, the last one ragged), K = 100 = three panels of 48 / 48 / 4 labels, so the 4-wide and
    the 8-wide walk both meet a `< K` tail, and a workspace for 8 parts: three parts of unequal fill, merged.  Seed 11: the fp64
    composition's smallest top-2 gap is 4.9e-3 at max|logit| 14.3 (2900 fp32 ulps) -- no ties; the run re-checks it on its own scores"""
    K, H, W = 100, 15, 15
    g, T, scale, _ = _op_case(B, K + 1, H, W, 11)
    T = T[:K].contiguous()                                                        # (without the builder's duplicate of a label: a tie)
    n = B * 16 * H * W
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    out2 = (C.c_int * 2)()
    for conf, part in ((0, 6), (1, 16)):
        _lib.check(lib.lseg_op_corr_argmax_ragged_split((C.c_int32 * B)(*([K] * B)), B, H, W, conf, 8 * n * part, cus, out2))
        assert out2[0] > 1 and out2[1] < K, "the workspace must force the label split"
    ws = torch.empty((8 * n * 16,), dtype=torch.uint8).cuda()
    a = dict(label=torch.full((B, 4 * H, 4 * W), -7, dtype=torch.int16).cuda(), score=torch.full((B, 4 * H, 4 * W), float("nan")).cuda())
    _lib.check(lib.lseg_op_corr_argmax(P(g), P(T), P(scale), P(a["label"]), P(a["score"]), B, K, H, W, 512, P(ws), 8 * n * 6, stream()))
    c = dict(label=torch.full_like(a["label"], -7), label2=torch.full_like(a["label"], -7),
             **{k: torch.full_like(a["score"], float("nan")) for k in ("score", "score2", "lse")})
    _lib.check(lib.lseg_op_corr_argmax_conf(P(g), P(T), P(scale), P(c["label"]), P(c["score"]), P(c["label2"]), P(c["score2"]), P(c["lse"]), B, K,
                                            H, W, 512, P(ws), 8 * n * 16, stream()))
    torch.cuda.synchronize()
    target = make_target(a["label"], K, 255, seed=11).cuda()                      # ignore_index, values >= K, label K - 1 of the last panel
    assert (target == 255).any() and ((target >= K) & (target != 255)).any() and (target == K - 1).any()
    run = _run(lib, g, T, scale, target, 255, B, K, H, W, parts=8)
    _same_bits_across_the_modes(a, c, {k: run.get(k) for k in ("label", "score", "lse")})
    assert (c["label"] >= 96).any(), "no winner in the last panel"


# ---- engine / network level ----------------------------------------------------------------------------------------------------------
def _tiny512():
    cfg = get_config("tiny16")
    return dataclasses.replace(cfg, out_c=512, text=dataclasses.replace(cfg.text, embed_dim=512))


def _engine_target(Bn, H, W, K, ign, seed):
    t = torch.randint(0, K, (Bn, H, W), generator=torch.Generator().manual_seed(seed), dtype=torch.int64)
    t[:, 0] = ign
    t[:, 1] = K + 1
    t[:, 2] = -7
    t[:, 3] = 0
    t[:, 4] = K - 1
    return t.cuda()


def test_streamed_forward_metrics_equal_forward_metrics(monkeypatch):
    """LSegNet.forward_metrics(streamed=True) on the widened small network (out_c 512: streamed), one shared set of 60 labels (two
    panels): the counts are forward_metrics()' exactly (both routes take the fused correlation's scale plane at K <= 157), nll_count
    too, nll_sum within n_valid x the lse bar measured on the network's own logits."""
    from modules.models.lseg_net import LSegNet
    cfg = _tiny512()
    monkeypatch.setitem(lseg_config._CONFIGS, "tiny16", cfg)
    labels = [f"thing {i}" for i in range(60)]
    net = LSegNet(labels=labels, backbone="tiny16", features=cfg.features, arch_option=0, block_depth=0, activation="lrelu")
    net.load_state_dict(synthetic_state_dict(net.cfg, seed=5))
    net = net.eval().cuda()
    x = synthetic_images(2, 64, 64, seed=5).cuda()
    target = _engine_target(2, 64, 64, 60, -1, seed=1)           # ignore_index -1: the rule of forward_stats and of label_stats coincide
    ref = net.forward_metrics(x, target, ignore_index=-1)
    r = net.forward_metrics(x, target, ignore_index=-1, streamed=True)
    assert set(r) == set(ref)
    for k in ("correct", "labeled", "nll_count"):
        assert r[k] == ref[k], k
    for k in ("area_inter", "area_pred", "area_lab", "area_union"):
        assert torch.equal(r[k], ref[k]), k
    with torch.no_grad():
        _, bar, own = _lse_bar(net(x))
    print(f"forward_metrics(streamed) K=60: nll_sum {r['nll_sum']:.6f} vs {ref['nll_sum']:.6f} over {r['nll_count']} pixels; lse bar {bar:.3e}")
    assert r["nll_count"] > 0 and abs(r["nll_sum"] - ref["nll_sum"]) <= r["nll_count"] * bar
    with pytest.raises(ValueError):
        net.forward_metrics(x, target, streamed=True, panel=16)


LISTS3 = [["cat", "grass"], ["road", "car", "sky", "tree", "other"], [f"thing {i}" for i in range(60)]]


def test_per_image_lists_equal_one_shared_set_run_per_list():
    """Eval mode, ragged lists of 2 / 5 / 60 labels: image b's loss, counts and planes against a shared-set forward_labels_loss of the SAME
    batch with list b (the tower is bit-identical), whose loss is in turn F.cross_entropy in double on the engine's own forward() logits
    within n_valid x the lse bar; the ragged counts are label_stats' on the ragged label map."""
    cfg = _tiny512()
    counts = [len(ls) for ls in LISTS3]
    Ksum = sum(counts)
    eng = HipEngine(cfg, 64, 64, max_batch=3, max_labels=Ksum, image_dtype="fp16")
    eng.load_state_dict(synthetic_state_dict(cfg, seed=5))
    tok = synthetic_tokens([lab for ls in LISTS3 for lab in ls], cfg.text.vocab, cfg.text.ctx)
    x = synthetic_images(3, 64, 64, seed=5).cuda()
    ign = -100
    target = torch.cat([_engine_target(1, 64, 64, k, ign, seed=b) for b, k in enumerate(counts)])
    eng.set_tokens(tok, group_sizes=counts)
    r = eng.forward_labels_loss(x, target, ign, plane=True)
    lab = eng.forward_labels(x)
    c2, _ = eng.label_stats(lab, target, ign)
    torch.cuda.synchronize()
    assert torch.equal(r["label"], lab) and torch.equal(r["counts"], c2) and r["counts"].numel() == 2 + 3 * Ksum
    total, nvalid, r0 = 0.0, 0, 0
    for b, k in enumerate(counts):
        eng.set_tokens(tok[r0:r0 + k])
        r0 += k
        tb = target.clone()
        one = eng.forward_labels_loss(x, tb, ign, plane=True)
        out = eng.forward(x)
        torch.cuda.synchronize()
        _, bar, _ = _lse_bar(out)
        valid = (tb[b] != ign) & (tb[b] >= 0) & (tb[b] < k)
        assert torch.equal(r["label"][b], one["label"][b]) and torch.equal(r["score"][b], one["score"][b])
        assert (r["nll_plane"][b].double() - one["nll_plane"][b].double()).abs().max().item() <= bar
        assert (r["nll_plane"][b][~valid] == 0).all()
        ce = F.cross_entropy(out[b:b + 1].double(), torch.where(valid, tb[b], torch.full_like(tb[b], ign))[None], ignore_index=ign, reduction="none")[0]
        d = (r["nll_plane"][b].double() - ce).abs().max().item()
        print(f"ragged eval image {b} (K={k}): max|nll - CE64(own logits)| {d:.3e}, lse bar {bar:.3e}")
        assert d <= bar
        total += ce.sum().item()
        nvalid += int(valid.sum())
    assert int(r["nll"][1].item()) == nvalid
    assert abs(r["nll"][0].item() - total) <= nvalid * bar
    eng.close()


def test_fallback_head_blocks_against_own_logits(golden_dir):
    """arch_option 1 (head blocks) cannot stream: the loss form of the reduction on the planes in memory, against F.cross_entropy in
    double on the engine's own forward() logits; label / score / lse are forward_labels_conf's."""
    g = torch.load(os.path.join(golden_dir, "ref_vitl16_96x96_k5_arch1.pt"))
    bb, H, W, Bn, K, seed, arch, depth = g["spec"]
    cfg = get_config(bb, arch_option=arch, block_depth=depth, activation="lrelu")
    eng = HipEngine(cfg, H, W, max_batch=Bn, max_labels=K, image_dtype="fp16")
    eng.load_state_dict(synthetic_state_dict(cfg, seed=seed))
    eng.set_tokens(g["tokens"])
    x = synthetic_images(Bn, H, W, seed=seed).cuda()
    ign = 255
    target = _engine_target(Bn, H, W, K, ign, seed=2)
    r = eng.forward_labels_loss(x, target, ign, plane=True)
    conf = eng.forward_labels_conf(x)
    out = eng.forward(x)
    c2, _ = eng.label_stats(conf["label"], target, ign)
    torch.cuda.synchronize()
    for k in ("label", "score", "lse"):
        assert torch.equal(r[k], conf[k]), k
    assert torch.equal(r["counts"], c2)
    valid = (target != ign) & (target >= 0) & (target < K)
    ce = F.cross_entropy(out.double(), torch.where(valid, target, torch.full_like(target, ign)), ignore_index=ign, reduction="none")
    _, bar, own = _lse_bar(out)
    d = (r["nll_plane"].double() - ce).abs().max().item()
    print(f"fallback arch1 K={K}: max|nll - CE64(own logits)| {d:.3e}, lse bar {bar:.3e}")
    assert d <= bar and (r["nll_plane"][~valid] == 0).all()
    nv = int(valid.sum())
    assert int(r["nll"][1].item()) == nv and abs(r["nll"][0].item() - ce.sum().item()) <= nv * bar
    eng.close()


def test_the_three_modes_of_the_fallback_agree_bit_for_bit():
    """the small network as it is (out_c 128 cannot stream): 100 labels on the (32, 32) logits in memory, the three modes of the fallback"""
    cfg = get_config("tiny16")
    K = 100
    eng = HipEngine(cfg, 64, 64, max_batch=2, max_labels=K, image_dtype="fp16")
    eng.load_state_dict(synthetic_state_dict(cfg, seed=3))
    eng.set_tokens(synthetic_tokens([f"thing {i}" for i in range(K)], cfg.text.vocab, cfg.text.ctx))
    x = synthetic_images(2, 64, 64, seed=3).cuda()
    label, score = eng.forward_labels(x, want_score=True)
    conf = eng.forward_labels_conf(x)
    loss = eng.forward_labels_loss(x, _engine_target(2, 64, 64, K, 255, seed=4), 255)
    torch.cuda.synchronize()
    _same_bits_across_the_modes(dict(label=label, score=score), conf, loss)
    eng.close()


def test_engine_entry_null_pointers_and_optional_outputs():
    cfg = _tiny512()
    eng = HipEngine(cfg, 64, 64, max_batch=1, max_labels=3, image_dtype="fp16")
    eng.load_state_dict(synthetic_state_dict(cfg, seed=0))
    eng.set_tokens(synthetic_tokens(["a", "b", "c"], cfg.text.vocab, cfg.text.ctx))
    x = synthetic_images(1, 64, 64, seed=0).cuda()
    target = _engine_target(1, 64, 64, 3, -1, seed=3)
    lab = torch.full((1, 64, 64), -7, dtype=torch.int16).cuda()
    nll = torch.full((2,), float("nan"), dtype=torch.float64).cuda()
    call = eng.lib.lseg_forward_labels_loss
    assert call(eng._h, P(x), 1, P(target), -1, None, None, None, None, P(nll), None, stream()) == -1       # NULL label output
    assert call(eng._h, P(x), 1, None, -1, P(lab), None, None, None, P(nll), None, stream()) == -1          # NULL target
    assert call(eng._h, None, 1, P(target), -1, P(lab), None, None, None, P(nll), None, stream()) == -1     # NULL input
    torch.cuda.synchronize()
    assert (lab == -7).all() and torch.isnan(nll).all()
    full = eng.forward_labels_loss(x, target, -1, plane=True)
    _lib.check(call(eng._h, P(x), 1, P(target), -1, P(lab), None, None, None, P(nll), None, stream()))      # only the sum beside the label
    torch.cuda.synchronize()
    assert torch.equal(lab, full["label"]) and torch.equal(nll, full["nll"]) and torch.equal(lab, eng.forward_labels(x))
    _lib.check(call(eng._h, P(x), 1, P(target), -1, P(lab), None, None, None, None, None, stream()))        # the label alone
    with pytest.raises(_lib.LSegError) as e:                                                                # streamed: no low-resolution logits
        eng.forward_stats(target)
    assert e.value.code == -4
    eng.close()
