"""Ragged per-image label sets in one batched forward (lseg_set_text_groups / lseg_op_corr_argmax_ragged, csrc/corr_argmax.hip RAGGED):
every image against its own list of labels, of its own length, labels local to that list.

  1. the op against the shared-set kernel: image b of ONE ragged launch == lseg_op_corr_argmax_conf with B = 1 on the image's slices --
     all five planes bit-equal without a workspace; with one (label parts sized from the largest list, short lists own fewer parts)
     the top-2 bit-equal and lse inside the bar tests/test_gpu_label_confidence.py applies between split and unsplit runs: 8 x the
     largest error fp32 torch.logsumexp itself shows against the fp64 one on the same planes
  2. the op against an fp64 composition per image, by the rule of tests/test_gpu_corr_argmax.py::test_corr_argmax_op_against_fp64
  3. the refusals, each before anything is launched
  4. the engine: ragged forward_labels_conf == three shared-set runs of the same batch, one per label list
  5. LSegNet.predict_labels with a list of label lists"""
import ctypes as C
import dataclasses
import functools

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

from lseg_hip import _lib                                                        # noqa: E402
from lseg_hip import config as lseg_config                                       # noqa: E402
from lseg_hip.config import get_config                                           # noqa: E402
from lseg_hip.engine import HipEngine                                            # noqa: E402
from lseg_hip.synth import synthetic_state_dict, synthetic_tokens, synthetic_images   # noqa: E402

GUARD = 64
PLANES_MAX_K = 157                       # lseg_op_corr_planes holds T in LDS: K <= 157 per call
NAMES = ("label", "score", "label2", "score2", "lse")


@pytest.fixture(scope="module")
def lib():
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    return _lib.load()


def P(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def ragged_case(counts, H, W, seed):
    """The recipe of tests/test_gpu_corr_argmax.py _op_case with one text block per image (CPU tensors): fp16 g / T with a decisive winner
    almost everywhere -- the base map of image b is made of 3 x 3 blocks, each the row of one label of ITS list (x an amplitude) + noise
    -- and the LAST label of every list of two or more duplicates the label of the image's block (0, 0): the first of the two must win
    every pixel either would, the duplicate is its runner-up.  The border of the padded map holds 1e3.  Returns g [B, H+2, W+2, 512],
    T [sum counts, 512], scale [B, 2H, 2W], the duplicated label of every image (None for a list of one)."""
    gen = torch.Generator().manual_seed(seed)
    B = len(counts)
    hb, wb = (H + 2) // 3, (W + 2) // 3
    Ts, labs, dups = [], [], []
    for k in counts:
        T = torch.randn((k, 512), generator=gen)
        T = T / T.norm(dim=-1, keepdim=True)
        lab = torch.randint(0, k - 1, (hb, wb), generator=gen) if k > 1 else torch.zeros((hb, wb), dtype=torch.long)
        if k > 1:
            T[k - 1] = T[lab[0, 0]]
        Ts.append(T.half())
        labs.append(lab.repeat_interleave(3, 0).repeat_interleave(3, 1)[:H, :W])
        dups.append(int(lab[0, 0]) if k > 1 else None)
    amp = 0.75 + 0.5 * torch.rand((B, H, W), generator=gen)
    rows = torch.stack([Ts[b].float()[labs[b]] for b in range(B)])
    gi = amp[..., None] * rows + 0.02 * torch.randn((B, H, W, 512), generator=gen)
    g = torch.full((B, H + 2, W + 2, 512), 1000.0)
    g[:, 1:H + 1, 1:W + 1] = gi
    scale = 8.0 + 4.0 * torch.rand((B, 2 * H, 2 * W), generator=gen)
    return g.half(), torch.cat(Ts), scale, dups


class Guarded:
    """the five outputs with NaN / -7 guard bands around each"""

    def __init__(self, B, H, W):
        self.n, self.shape = B * 16 * H * W, (B, 4 * H, 4 * W)
        self.buf = {k: (torch.full((self.n + 2 * GUARD,), -7, dtype=torch.int16) if k.startswith("label")
                        else torch.full((self.n + 2 * GUARD,), float("nan"))).cuda() for k in NAMES}

    def ptrs(self):
        return [P(self.buf[k][GUARD:]) for k in NAMES]

    def get(self, k):
        return self.buf[k][GUARD:GUARD + self.n].view(self.shape)

    def untouched(self):
        return all(((b == -7) if k.startswith("label") else torch.isnan(b)).all() for k, b in self.buf.items())

    def check_guards(self):
        for k, b in self.buf.items():
            ok = (lambda t: (t == -7).all()) if k.startswith("label") else (lambda t: torch.isnan(t).all())
            assert ok(b[:GUARD]) and ok(b[-GUARD:]), f"{k}: written outside the output"
            if not k.startswith("label"):
                assert not torch.isnan(self.get(k)).any(), f"{k}: an output pixel was not written"


def _ragged(lib, g, T, scale, counts, H, W, ws_parts=0):
    B = len(counts)
    out = Guarded(B, H, W)
    off = torch.full((B + 1 + 2 * GUARD,), -7, dtype=torch.int32).cuda()
    ws_bytes = ws_parts * out.n * 16
    ws = torch.zeros((ws_bytes + 4 * GUARD,), dtype=torch.uint8).cuda() if ws_parts else None
    _lib.check(lib.lseg_op_corr_argmax_ragged(P(g), P(T), P(scale), (C.c_int32 * B)(*counts), P(off[GUARD:]), *out.ptrs(), B, H, W, 512,
                                              P(ws), ws_bytes, stream()))
    torch.cuda.synchronize()
    out.check_guards()
    assert (off[:GUARD] == -7).all() and (off[GUARD + B + 1:] == -7).all(), "offsets: written outside the B + 1 entries"
    assert off[GUARD:GUARD + B + 1].tolist() == [sum(counts[:b]) for b in range(B + 1)]
    if ws is not None:
        assert (ws[ws_bytes:] == 0).all(), "workspace: written beyond ws_bytes"
    return out


def _shared_b1(lib, g, T, scale, K, H, W):
    out = Guarded(1, H, W)
    _lib.check(lib.lseg_op_corr_argmax_conf(P(g), P(T), P(scale), *out.ptrs(), 1, K, H, W, 512, None, 0, stream()))
    torch.cuda.synchronize()
    out.check_guards()
    return out


def _fp64_composition(g, T, scale, H, W):
    R = torch.einsum("kc,byxc->bkyx", T.double(), g[:, 1:H + 1, 1:W + 1].double())
    mid = F.interpolate(R, scale_factor=2, mode="bilinear", align_corners=True) * scale.double().unsqueeze(1)
    return F.interpolate(mid, scale_factor=2, mode="bilinear", align_corners=True)


def _planes(lib, g, T, scale, K, H, W):
    """the full-resolution logits of one image from the project's own plane kernels (tests/test_gpu_label_confidence.py _planes)"""
    chunks = []
    for k0 in range(0, K, PLANES_MAX_K):
        kc = min(PLANES_MAX_K, K - k0)
        R = torch.zeros((1, kc, (H + 2) * (W + 2)), device="cuda")
        _lib.check(lib.lseg_op_corr_planes(P(g), P(T[k0:k0 + kc].contiguous()), P(R), None, 1, kc, H, W, 512, stream()))
        chunks.append(R)
    R = torch.cat(chunks, 1).contiguous()
    out = torch.empty((1, K, 4 * H, 4 * W), device="cuda")
    _lib.check(lib.lseg_op_upsample4x_planes_scaled(P(R), P(scale), P(out), 1, K, H, W, 0, None, stream()))
    torch.cuda.synchronize()
    return out


def _lse_bar(planes):
    """tests/test_gpu_label_confidence.py _lse_bar: (8 x the error of fp32 torch.logsumexp against the fp64 one, that error)"""
    ref = torch.logsumexp(planes.double(), 1)
    own = (torch.logsumexp(planes, 1).double() - ref).abs().max().item()
    return 8.0 * own, own


@functools.lru_cache(maxsize=None)
def _case(counts, H, W, seed):
    """inputs, the ragged runs (without / with a workspace) and the per-image references of one case: computed once, shared, never modified"""
    lib = _lib.load()
    g, T, scale, dups = (t.cuda() if isinstance(t, torch.Tensor) else t for t in ragged_case(counts, H, W, seed))
    plain = _ragged(lib, g, T, scale, counts, H, W)
    split = _ragged(lib, g, T, scale, counts, H, W, ws_parts=8)
    refs, bars = [], []
    for b, k in enumerate(counts):
        r0 = sum(counts[:b])
        gb, Tb, sb = g[b:b + 1].contiguous(), T[r0:r0 + k].contiguous(), scale[b:b + 1].contiguous()
        refs.append(_shared_b1(lib, gb, Tb, sb, k, H, W))
        # as there: the plane kernels need an even W; where they cannot form the planes the bar is measured the same way on the fp64
        # composition rounded to fp32
        planes = _planes(lib, gb, Tb, sb, k, H, W) if W % 2 == 0 else _fp64_composition(gb, Tb, sb, H, W).float()
        bars.append(_lse_bar(planes))
    return dict(g=g, T=T, scale=scale, dups=dups, plain=plain, split=split, refs=refs, bars=bars)


# (counts; H x W; seed): one tile and the single-label rule; lists straddling one panel beside a 7-panel one on an odd map; nine tiles with
# ragged edges, lists of 2 .. 1000 labels (21 panels) straddling corr_planes' LDS limit
CASES = [((1, 16, 49), 6, 6, 1), ((47, 48, 300), 9, 17, 4), ((2, 157, 158, 1000), 30, 30, 3)]


@pytest.mark.gpu_fast
@pytest.mark.parametrize("counts,H,W,seed", CASES)
def test_every_image_is_bit_equal_to_the_shared_set_kernel_on_its_own_slices(lib, counts, H, W, seed):
    c = _case(counts, H, W, seed)
    for b, k in enumerate(counts):
        ref = c["refs"][b]
        for name in NAMES:                                                     # no workspace: all five planes, bit for bit
            assert torch.equal(c["plain"].get(name)[b], ref.get(name)[0]), (b, k, name)
        for name in ("label", "score", "label2", "score2"):                    # label parts: top-2 by the same rule
            assert torch.equal(c["split"].get(name)[b], ref.get(name)[0]), (b, k, name, "workspace")
        d = (c["split"].get("lse")[b].double() - ref.get("lse")[0].double()).abs().max().item()
        bar, own = c["bars"][b]
        print(f"ragged op counts={counts} {H}x{W} image {b} (K={k}): max|lse(split) - lse| {d:.3e}, bar {bar:.3e} "
              f"(fp32 torch.logsumexp vs fp64: {own:.3e})")
        assert d <= bar
        for run in (c["plain"], c["split"]):                                   # labels local to the image's own list
            lab, lab2 = run.get("label")[b], run.get("label2")[b]
            assert (lab >= 0).all() and (lab < k).all()
            if k == 1:                                                         # as K = 1: no runner-up, lse = score
                assert (lab2 == -1).all() and torch.isinf(run.get("score2")[b]).all() and (run.get("score2")[b] < 0).all()
                assert torch.equal(run.get("lse")[b], run.get("score")[b])
            else:
                assert (lab2 >= 0).all() and (lab2 < k).all() and (lab2 != lab).all()
                assert torch.isfinite(run.get("score2")[b]).all() and torch.isfinite(run.get("lse")[b]).all()
                won = lab == c["dups"][b]                                      # the duplicated last label is the runner-up of the original
                assert won.any() and (lab2[won] == k - 1).all() and (lab != k - 1).all()


@pytest.mark.gpu_fast
def test_plain_argmax_instantiation_without_the_confidence_outputs(lib):
    """the last three outputs NULL: the arg-max instantiation, same label and score -- without and with label parts"""
    counts, H, W, seed = CASES[1]
    c = _case(counts, H, W, seed)
    B, n = len(counts), len(counts) * 16 * H * W
    off = torch.zeros((B + 1,), dtype=torch.int32).cuda()
    for parts in (0, 8):
        lab = torch.full((B, 4 * H, 4 * W), -7, dtype=torch.int16).cuda()
        sc = torch.full((B, 4 * H, 4 * W), float("nan")).cuda()
        ws = torch.empty((parts * n * 6,), dtype=torch.uint8).cuda() if parts else None
        _lib.check(lib.lseg_op_corr_argmax_ragged(P(c["g"]), P(c["T"]), P(c["scale"]), (C.c_int32 * B)(*counts), P(off), P(lab), P(sc), None, None,
                                                  None, B, H, W, 512, P(ws), parts * n * 6, stream()))
        torch.cuda.synchronize()
        assert torch.equal(lab, c["plain"].get("label")) and torch.equal(sc, c["plain"].get("score"))


FP64_CASE = ((47, 48, 300), 9, 17, 49)       # 3 of the 7 344 pixels are that close in fp64 (seeds 1 .. 59 leave 3 .. 14)


@pytest.mark.gpu_fast
def test_ragged_op_against_fp64_per_image(lib):
    """tests/test_gpu_corr_argmax.py::test_corr_argmax_op_against_fp64, per image of one ragged launch: labels must agree wherever the fp64
    top-2 margin exceeds 2x the measured max |score - fp64 value|; at most 0.1 % of the pixels may be excluded; the score error is at most
    2e-3 of the largest |value|.  (The seed is one for which the fp64 composition alone leaves <= 0.1 % of the pixels with a top-2
    margin under 4x the fp16 rounding of the (2h, 2w) logits, chosen on the CPU.)"""
    counts, H, W, seed = FP64_CASE
    c = _case(counts, H, W, seed)
    label, score = c["plain"].get("label"), c["plain"].get("score")
    refs = []
    for b, k in enumerate(counts):
        r0 = sum(counts[:b])
        ref = _fp64_composition(c["g"][b:b + 1], c["T"][r0:r0 + k], c["scale"][b:b + 1], H, W)[0]
        assert (ref[k - 1] - ref[c["dups"][b]]).abs().max().item() == 0.0
        refs.append(ref[:k - 1].topk(2, dim=0))                                 # tie rule: the reference is taken without the duplicate
    ref_val = torch.stack([t.values[0] for t in refs])
    ref_am = torch.stack([t.indices[0] for t in refs])
    margin = torch.stack([t.values[0] - t.values[1] for t in refs])
    err = (score.double() - ref_val).abs().max().item()
    decisive = margin > 2 * err
    excluded = 1.0 - decisive.double().mean().item()
    print(f"ragged op counts={counts} {H}x{W}: max|score - fp64| {err:.3e}, excluded (margin <= 2 err) {excluded:.5f}, "
          f"mismatches at decisive pixels {(label.long()[decisive] != ref_am[decisive]).sum().item()}")
    assert err <= 2e-3 * ref_val.abs().max().item(), err
    assert excluded <= 1e-3, excluded
    assert torch.equal(label.long()[decisive], ref_am[decisive])


@pytest.mark.gpu_fast
def test_refusals_launch_nothing(lib):
    H = W = 4
    g = torch.zeros((2, H + 2, W + 2, 512), dtype=torch.float16).cuda()
    T = torch.zeros((64, 512), dtype=torch.float16).cuda()
    sc = torch.ones((2, 2 * H, 2 * W)).cuda()
    off = torch.full((3,), -7, dtype=torch.int32).cuda()
    o = Guarded(2, H, W)
    call = lib.lseg_op_corr_argmax_ragged
    cnt = lambda *v: (C.c_int32 * len(v))(*v)                                  # noqa: E731
    tail = (2, H, W, 512, None, 0, stream())
    assert call(P(g), P(T), P(sc), cnt(3, 0), P(off), *o.ptrs(), *tail) == -1                   # a count < 1: LSEG_ERR_INVALID
    assert call(P(g), P(T), P(sc), cnt(-2, 3), P(off), *o.ptrs(), *tail) == -1
    assert call(P(g), P(T), P(sc), cnt(3, 32768), P(off), *o.ptrs(), *tail) == -1               # a count > 32767
    assert b"32767" in lib.lseg_last_error(None)
    assert call(None, P(T), P(sc), cnt(3, 5), P(off), *o.ptrs(), *tail) == -1                   # NULL required pointers
    assert call(P(g), None, P(sc), cnt(3, 5), P(off), *o.ptrs(), *tail) == -1
    assert call(P(g), P(T), None, cnt(3, 5), P(off), *o.ptrs(), *tail) == -1
    assert call(P(g), P(T), P(sc), None, P(off), *o.ptrs(), *tail) == -1
    assert call(P(g), P(T), P(sc), cnt(3, 5), None, *o.ptrs(), *tail) == -1
    assert call(P(g), P(T), P(sc), cnt(3, 5), P(off), None, *o.ptrs()[1:], *tail) == -1
    assert call(P(g), P(T), P(sc), cnt(3, 5), P(off), *o.ptrs(), 2, H, W, 768, None, 0, stream()) == -5    # other widths: LSEG_ERR_UNSUPPORTED
    assert call(P(g), P(T), P(sc), cnt(3, 5), P(off), *o.ptrs(), 2, 1, W, 512, None, 0, stream()) == -1    # the bilinear needs 2 rows
    torch.cuda.synchronize()
    assert o.untouched() and (off == -7).all(), "a refused call wrote something"
    _lib.check(call(P(g), P(T), P(sc), cnt(3, 5), P(off), *o.ptrs(), *tail))                    # and the same call with good counts runs
    torch.cuda.synchronize()
    o.check_guards()
    assert off.tolist() == [0, 3, 8]


# ---- engine / network level ----------------------------------------------------------------------------------------------------------
COUNTS3 = (2, 5, 9)
LISTS3 = [["cat", "grass"], ["road", "car", "sky", "tree", "other"], [f"thing {i}" for i in range(9)]]


def _tiny512():
    cfg = get_config("tiny16")
    return dataclasses.replace(cfg, out_c=512, text=dataclasses.replace(cfg.text, embed_dim=512))


def _equal_within_bar(r, ref, b, bar):
    for k in ("label", "score", "label2", "score2"):
        assert torch.equal(r[k][b], ref[k][b]), (b, k)
    d = (r["lse"][b].double() - ref["lse"][b].double()).abs().max().item()
    assert d <= bar, (b, d, bar)
    return d


@pytest.mark.gpu_fast
def test_engine_ragged_equals_one_shared_set_run_per_label_list(lib):
    """The synthetic small network widened to out_c = 512 (commuted schedule: streamed), B = 3, lists of 2 / 5 / 9 labels: image b of the
    ragged forward_labels_conf == image b of a shared-set forward_labels_conf of the SAME batch with list b (same B: the tower is
    bit-identical).  The ragged state refuses logits (LSEG_ERR_UNSUPPORTED) and has no planes (LSEG_ERR_STATE); clearing the groups
    gives the shared-set results back."""
    cfg = _tiny512()
    K = sum(COUNTS3)
    eng = HipEngine(cfg, 64, 64, max_batch=3, max_labels=K, image_dtype="fp16")
    eng.load_state_dict(synthetic_state_dict(cfg, seed=5))
    tok = synthetic_tokens([lab for ls in LISTS3 for lab in ls], cfg.text.vocab, cfg.text.ctx)
    x = synthetic_images(3, 64, 64, seed=5).cuda()
    eng.set_tokens(tok)
    before = eng.forward_labels_conf(x)                                         # all 16 labels shared by the batch
    shared, bars = [], []
    for b, k in enumerate(COUNTS3):
        r0 = sum(COUNTS3[:b])
        eng.set_tokens(tok[r0:r0 + k])
        shared.append(eng.forward_labels_conf(x))
        bars.append(_lse_bar(eng.forward(x))[0])
    eng.set_tokens(tok, group_sizes=COUNTS3)
    r = eng.forward_labels_conf(x)
    lab, score = eng.forward_labels(x, want_score=True)
    torch.cuda.synchronize()
    assert torch.equal(lab, r["label"]) and torch.equal(score, r["score"])
    for b, k in enumerate(COUNTS3):
        d = _equal_within_bar(r, shared[b], b, bars[b])
        print(f"engine ragged image {b} (K={k}): max|lse - lse(shared-set run)| {d:.3e}, bar {bars[b]:.3e}")
        assert (r["label"][b] >= 0).all() and (r["label"][b] < k).all() and (r["label2"][b] < k).all()
    # nothing but the streamed labels exists for ragged groups
    logits = torch.full((3, K, 64, 64), float("nan")).cuda()
    assert eng.lib.lseg_forward(eng._h, P(x), 3, P(logits), None, stream()) == -5            # LSEG_ERR_UNSUPPORTED
    assert b"ragged" in eng.lib.lseg_last_error(None)
    torch.cuda.synchronize()
    assert torch.isnan(logits).all()
    with pytest.raises(_lib.LSegError) as e:
        eng.forward(x)
    assert e.value.code == -5
    with pytest.raises(_lib.LSegError) as e:
        eng.forward_lowres(x)
    assert e.value.code == -5
    eng.forward_labels(x)
    with pytest.raises(_lib.LSegError) as e:
        eng.forward_stats(torch.zeros((3, 64, 64), dtype=torch.long).cuda())
    assert e.value.code == -4 and "labels-only" in str(e.value)                              # LSEG_ERR_STATE
    with pytest.raises(_lib.LSegError) as e:
        eng.intermediate("lowres", (3, K, 32, 32))
    assert e.value.code == -4
    # another batch size, or counts that do not add up to K: LSEG_ERR_INVALID
    lab2 = torch.empty((2, 64, 64), dtype=torch.int16).cuda()
    assert eng.lib.lseg_forward_labels(eng._h, P(x), 2, P(lab2), None, stream()) == -1
    bad = (C.c_int32 * 3)(2, 5, 8)
    _lib.check(eng.lib.lseg_set_text_groups(eng._h, bad, 3))
    assert eng.lib.lseg_forward_labels(eng._h, P(x), 3, P(lab), None, stream()) == -1
    assert eng.lib.lseg_set_text_groups(eng._h, (C.c_int32 * 3)(2, 0, 14), 3) == -1
    # either grouping clears the other; cleared, the shared set is what it was
    _lib.check(eng.lib.lseg_set_text_groups(eng._h, (C.c_int32 * 3)(*COUNTS3), 3))
    _lib.check(eng.lib.lseg_set_text_grouping(eng._h, 0))
    eng._groups = None
    after = eng.forward_labels_conf(x)
    for k in NAMES:
        assert torch.equal(after[k], before[k]), k
    eng.set_tokens(tok, group_sizes=COUNTS3)
    eng.set_tokens(tok)                                                                      # group_sizes=None clears
    after = eng.forward_labels_conf(x)
    torch.cuda.synchronize()
    for k in NAMES:
        assert torch.equal(after[k], before[k]), k
    eng.close()


@pytest.mark.gpu_fast
def test_ragged_groups_over_external_text_features(lib):
    """lseg_set_text_features + group sizes (a label bank of an application): image b == the shared-set run over its slice of the rows"""
    cfg = _tiny512()
    K = sum(COUNTS3)
    eng = HipEngine(cfg, 64, 64, max_batch=3, max_labels=K, image_dtype="fp16")
    eng.load_state_dict(synthetic_state_dict(cfg, seed=5))
    x = synthetic_images(3, 64, 64, seed=5).cuda()
    feat = torch.randn((K, 512), generator=torch.Generator().manual_seed(9)).half().cuda()
    eng.set_text_features(feat, group_sizes=COUNTS3)
    r = eng.forward_labels_conf(x)
    for b, k in enumerate(COUNTS3):
        r0 = sum(COUNTS3[:b])
        eng.set_text_features(feat[r0:r0 + k])
        assert eng._groups is None
        ref = eng.forward_labels_conf(x)
        _equal_within_bar(r, ref, b, _lse_bar(eng.forward(x))[0])
    eng.close()


def test_predict_labels_with_one_label_list_per_image(monkeypatch):
    """LSegNet.predict_labels(x, [[..], [..], [..]]) on the widened small network == the engine-level ragged result as torch.long; with
    confidence=True prob / margin follow from the planes as in the shared-set case; a flat list keeps its meaning."""
    from modules.models.lseg_net import LSegNet
    cfg = _tiny512()
    monkeypatch.setitem(lseg_config._CONFIGS, "tiny16", cfg)
    net = LSegNet(labels=["a", "b"], backbone="tiny16", features=cfg.features, arch_option=0, block_depth=0, activation="lrelu")
    assert net.cfg.out_c == 512
    net.load_state_dict(synthetic_state_dict(net.cfg, seed=5))
    net = net.eval().cuda()
    x = synthetic_images(3, 64, 64, seed=5).cuda()
    plain = net.predict_labels(x, LISTS3)
    r = net.predict_labels(x, LISTS3, confidence=True)
    eng = net._last_engine
    assert eng._groups == list(COUNTS3)
    e = eng.forward_labels_conf(x)
    torch.cuda.synchronize()
    assert plain.dtype == torch.long and plain.shape == (3, 64, 64) and torch.equal(plain, e["label"].long())
    assert set(r) == {"label", "prob", "label2", "margin"}
    assert torch.equal(r["label"], plain) and torch.equal(r["label2"], e["label2"].long())
    assert torch.equal(r["prob"], torch.exp(e["score"] - e["lse"])) and torch.equal(r["margin"], e["score"] - e["score2"])
    assert (r["prob"] > 0).all() and (r["prob"] <= 1).all() and (r["margin"] >= 0).all()
    for b, k in enumerate(COUNTS3):
        assert int(plain[b].max()) < k
    # one flat list: a label set shared by the batch, as before -- and the groups are gone
    flat = net.predict_labels(x, LISTS3[2])
    assert net._last_engine._groups is None and flat.shape == (3, 64, 64) and int(flat.max()) < 9
    with torch.no_grad():
        out = net(x, LISTS3[2])
    top2 = out.topk(2, dim=1)
    decisive = (top2.values[:, 0] - top2.values[:, 1]) > 1e-6
    assert torch.equal(flat[decisive], top2.indices[:, 0][decisive])
    with pytest.raises(ValueError):
        net.predict_labels(x, LISTS3[:2])                                                    # two lists for three images
