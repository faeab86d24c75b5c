"""Host side of the few-shot episode evaluation (no GPU): the plain-torch helper against the fixtures recorded from the reference's own
Evaluator (tools/make_ref_episode_golden.py), EpisodeMeter's formulas, the module's batch layouts and the C declarations."""
import os
import re

import pytest
import torch

import episode_helpers as eh
from lseg_hip import _lib
from lseg_hip.episode import EpisodeMeter, NCLASS

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
FIXTURES = sorted(f[:-3] for f in os.listdir(GOLD) if f.startswith("ref_episode_"))
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def load_fixture(name):
    fx = torch.load(os.path.join(GOLD, name + ".pt"))
    return fx, fx["scores_f16"].float(), fx["target_u8"].long(), fx["ignore_u8"]


def test_fixture_set_is_complete():
    assert FIXTURES == ["ref_episode_96x96_b1", "ref_episode_9x11_b3"]
    fx, scores, target, ignore = load_fixture("ref_episode_9x11_b3")
    assert scores.shape == (3, 2, 9, 11)
    assert (scores[0, 0] == scores[0, 1]).sum() >= 4                              # exact ties
    assert int(fx["area_inter_noignore"][:, 1].sum()) == 0                        # image 1 never meets its target
    assert bool(ignore[2].all()) and int(fx["area_union_ignore"][:, 2].sum()) == 0   # image 2 ignored entirely
    assert load_fixture("ref_episode_96x96_b1")[1].shape == (1, 2, 96, 96)


@pytest.mark.parametrize("name", FIXTURES)
@pytest.mark.parametrize("tag", ["ignore", "noignore"])
def test_helper_equals_reference_evaluator(name, tag):
    fx, scores, target, ignore = load_fixture(name)
    areas = eh.classify(eh.predict(scores), target, ignore if tag == "ignore" else None)
    inter, union = eh.inter_union(areas)
    assert torch.equal(inter, fx[f"area_inter_{tag}"]) and torch.equal(union, fx[f"area_union_{tag}"])
    assert torch.equal(eh.predict(scores), scores.argmax(1))                       # a tie is class 0
    assert eh.flags(target, ignore).tolist() == [0, 0]


def test_helper_cross_entropy_is_torch_cross_entropy():
    _, scores, target, _ = load_fixture("ref_episode_9x11_b3")
    t = target.clone()
    t[0, 0, :3] = -100
    s, n = eh.cross_entropy(scores, t)
    ref = torch.nn.functional.cross_entropy(scores.double().view(3, 2, -1), t.view(3, -1))
    assert abs(float(s.sum() / n.sum()) - float(ref)) <= 1e-12 * abs(float(ref))
    assert int(n.sum()) == t.numel() - 3


def test_meter_formulas_union_zero_and_duplicate_ids():
    m = EpisodeMeter(6, [0, 2, 3, 5], device="cpu")
    h = eh.Meter(6, [0, 2, 3, 5])
    inter = torch.tensor([[5, 0, 7, 11], [3, 0, 2, 1]])
    union = torch.tensor([[9, 4, 7, 30], [8, 6, 2, 13]])
    ids = [2, 5, 2, 0]                                                            # class 2 twice; class 3 of interest stays at union 0
    m.update(inter, union, torch.tensor(ids), torch.tensor(0.5))
    m.update(inter[:, :1], union[:, :1], [5], None)
    h.update(inter, union, ids)
    h.update(inter[:, :1], union[:, :1], [5])
    assert torch.equal(m.intersection_buf, h.inter) and torch.equal(m.union_buf, h.union)
    assert m.intersection_buf[:, 2].tolist() == [12, 5] and m.union_buf[:, 3].tolist() == [0, 0]
    miou, fb = m.compute_iou()
    rm, rf = h.compute_iou()
    assert miou.dtype == torch.float32 and fb.dtype == torch.float32
    assert abs(float(miou) - rm) <= 1e-6 * rm and abs(float(fb) - rf) <= 1e-6 * rf
    assert len(m.loss_buf) == 2 and all(x.dim() == 0 for x in m.loss_buf)
    m.reset()
    assert int(m.intersection_buf.sum()) == 0 and int(m.union_buf.sum()) == 0 and m.loss_buf == []


@pytest.mark.parametrize("which", [0, 1])
def test_compute_iou_raises_on_flags(which):
    m = EpisodeMeter("pascal", list(range(5)), device="cpu")
    f = torch.zeros(2, dtype=torch.int64)
    f[which] = 3
    m.update(torch.ones(2, 1, dtype=torch.int64), torch.ones(2, 1, dtype=torch.int64) * 2, [1], None, flags=f)
    with pytest.raises(ValueError, match="3 pixels"):
        m.compute_iou()
    m.reset()
    m.update(torch.ones(2, 1, dtype=torch.int64), torch.ones(2, 1, dtype=torch.int64) * 2, [1], None)
    m.compute_iou()


def test_nclass_per_benchmark():
    assert NCLASS == {"pascal": 20, "coco": 80, "fss": 1000}
    for name, n in NCLASS.items():
        m = EpisodeMeter(name, [0, n - 1], device="cpu")
        assert m.nclass == n and m.intersection_buf.shape == (2, n) and m.intersection_buf.dtype == torch.int64
    assert EpisodeMeter(7, [6], device="cpu").nclass == 7
    with pytest.raises(ValueError):
        EpisodeMeter("ade20k", [0], device="cpu")
    with pytest.raises(ValueError):
        EpisodeMeter("pascal", [20], device="cpu")


def _module(dataset, **kw):
    from modules.lsegmentation_module_zs import LSegmentationModuleZS
    return LSegmentationModuleZS("nowhere", dataset, 2, 0.004, 10, **kw)


def test_validation_batch_inputs_both_layouts():
    H, W = 4, 6
    g = torch.Generator().manual_seed(3)
    # 5-shot finetune: [bsz, 5, ...] viewed as [bsz * 5, ...], class_id repeated shot-major as the reference does
    batch = {"query_img": torch.randn(2, 5, 3, H, W, generator=g), "query_mask": torch.randint(0, 2, (2, 5, H, W), generator=g),
             "query_ignore_idx": torch.randint(0, 2, (2, 5, H, W), generator=g), "class_id": torch.tensor([3, 8])}
    m = _module("pascal", finetune_mode=True, nshot=5)
    img, target, ci, ig = m.validation_batch_inputs(batch)
    assert img.shape == (10, 3, H, W) and target.shape == (10, H, W) and ig.shape == (10, H, W)
    assert ci.tolist() == [3, 8] * 5
    assert torch.equal(img[7], batch["query_img"][1, 2]) and torch.equal(ig[7], batch["query_ignore_idx"][1, 2])
    assert _module("coco", finetune_mode=True, nshot=5).validation_batch_inputs(batch)[3] is None     # the 'pascal' rule
    # query layout
    q = {"query_img": torch.randn(2, 1, 3, H, W, generator=g), "query_mask": torch.randint(0, 2, (2, 1, H, W), generator=g),
         "query_ignore_idx": torch.randint(0, 2, (2, 1, H, W), generator=g), "class_id": torch.tensor([1, 1])}
    for kw in (dict(finetune_mode=False, nshot=1), dict(finetune_mode=True, nshot=1)):
        img, target, ci, ig = _module("pascal", **kw).validation_batch_inputs(q)
        assert img.shape == (2, 3, H, W) and target.shape == (2, H, W) and ci.tolist() == [1, 1]
        assert torch.equal(ig, q["query_ignore_idx"].squeeze(1))
    q2 = {k: v for k, v in q.items() if k != "query_ignore_idx"}
    assert _module("pascal").validation_batch_inputs(q2)[3] is None                # no mask in the batch
    assert _module("fss").validation_batch_inputs(q)[3] is None


def test_training_step_without_a_meter_logs_what_it_logged():
    m = _module("fss", finetune_mode=True, nshot=1)
    logged, calls = [], []

    class Net:
        def forward_loss(self, img, class_info, t, ignore_index):
            calls.append((tuple(img.shape), class_info.tolist(), tuple(t.shape), t.dtype, ignore_index))
            return torch.tensor(0.25)

    object.__setattr__(m, "net", Net())
    m.log = lambda *a, **k: logged.append((a, k))
    batch = {"support_imgs": torch.zeros(2, 1, 3, 4, 4), "support_masks": torch.zeros(2, 1, 4, 4), "class_id": torch.tensor([5, 6])}
    loss = m.training_step(batch, 0)
    assert float(loss) == 0.25 and len(logged) == 1 and logged[0][0][0] == "train_loss" and logged[0][0][1] is loss and logged[0][1] == {}
    assert calls == [((2, 3, 4, 4), [5, 6], (2, 4, 4), torch.int64, -100)]
    assert not hasattr(m, "train_average_meter")


def test_new_symbols_are_declared():
    header = open(os.path.join(ROOT, "include", "lseg_hip.h")).read()
    for name, nargs in (("lseg_op_episode_stats", 18), ("lseg_op_episode_stats_ws_bytes", 3), ("lseg_episode_stats", 12)):
        assert name in _lib.SIGNATURES and len(_lib.SIGNATURES[name][1]) == nargs
        decl = re.search(r"\b(?:int|size_t) " + name + r"\(([^;]*)\);", header)
        assert decl is not None and decl.group(1).count(",") + 1 == nargs, name
    lib = _lib.load()
    assert lib.lseg_abi_version() == _lib.ABI_VERSION
    assert lib.lseg_op_episode_stats_ws_bytes(3, 9, 11) >= 3 * 16 and lib.lseg_op_episode_stats_ws_bytes(0, 9, 11) == 0
