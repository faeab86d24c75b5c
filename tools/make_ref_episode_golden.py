"""tests/golden/ref_episode_*.pt -- few-shot episode areas recorded from the REFERENCE'S OWN Evaluator.  TEST INFRASTRUCTURE, build
container only (needs the reference checkout that oracle/make_ref_golden.py loads).

Imports the reference's fewshot_data/common/evaluation.py from where it lies and calls Evaluator.classify_prediction(pred, target,
ignore) on seeded inputs, on the CPU, with float masks (torch.histc has no int64 CPU kernel; the function itself is dtype-agnostic).
AverageMeter is NOT driven: its constructor calls .cuda() and its module imports tensorboardX; the meter is tested against
tests/episode_helpers.py instead.

Every fixture stores the inputs compactly (scores as fp16 -- every value is fp16-representable, so .float() is exact --, target / ignore
as uint8, class ids) and the recorded [2, B] area_inter / area_union WITH and WITHOUT the ignore mask.  Cases:
  ref_episode_9x11_b3   image 0: random, an ignored band (target 0 there), exact ties v0 == v1 on a block;
                        image 1: the prediction never meets the target and nothing is ignored (the reference's empty-intersection branch);
                        image 2: ignored entirely
  ref_episode_96x96_b1  one image of 9216 pixels (spans several workgroups), an ignored band and ties

    python tools/make_ref_episode_golden.py [--reference DIR]
"""
import argparse
import importlib.util
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle.make_ref_golden import REF          # noqa: E402  (where the reference checkout lies in the build container)

GOLD = os.path.join(ROOT, "tests", "golden")


def reference_evaluator(ref):
    spec = importlib.util.spec_from_file_location("ref_fewshot_evaluation", os.path.join(ref, "fewshot_data", "common", "evaluation.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    mod.Evaluator.initialize()
    return mod.Evaluator


def make_inputs(B, H, W, seed):
    g = torch.Generator().manual_seed(seed)
    scores = (torch.randn(B, 2, H, W, generator=g) * 3).half().float()
    target = torch.randint(0, 2, (B, H, W), generator=g)
    ignore = torch.zeros(B, H, W, dtype=torch.uint8)
    # image 0: an ignored band (target 0 under it, as the loaders guarantee) and a block of exact ties over both target values
    ignore[0, H // 3:H // 3 + max(1, H // 6), 1:W - 1] = 1
    scores[0, 1, -max(2, H // 4):, :W // 2] = scores[0, 0, -max(2, H // 4):, :W // 2]
    if B > 1:                                   # image 1: pred = 1 - target everywhere, nothing ignored
        scores[1, 0] = target[1].float() * 2 - 1
        scores[1, 1] = -scores[1, 0]
    if B > 2:                                   # image 2: ignored entirely
        ignore[2] = 1
    target[ignore != 0] = 0
    return scores, target, ignore


def record(Evaluator, scores, target, ignore):
    out = {}
    for tag, ig in (("ignore", ignore), ("noignore", None)):
        pred = scores.argmax(dim=1).float()                                   # out.argmax(dim=1): first maximum wins
        inter, union = Evaluator.classify_prediction(pred.clone(), target.float().clone(), None if ig is None else ig.float().clone())
        assert inter.shape == (2, scores.shape[0]) and union.shape == inter.shape
        assert torch.equal(inter, inter.round()) and torch.equal(union, union.round())
        out[f"area_inter_{tag}"] = inter.long()
        out[f"area_union_{tag}"] = union.long()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", default=os.environ.get("LSEG_REFERENCE", REF))
    args = ap.parse_args()
    Evaluator = reference_evaluator(args.reference)
    for name, (B, H, W, seed, ids) in {"ref_episode_9x11_b3": (3, 9, 11, 41, [4, 17, 4]), "ref_episode_96x96_b1": (1, 96, 96, 42, [9])}.items():
        scores, target, ignore = make_inputs(B, H, W, seed)
        assert torch.equal(scores.half().float(), scores)
        fx = {"scores_f16": scores.half(), "target_u8": target.to(torch.uint8), "ignore_u8": ignore, "class_id": torch.tensor(ids),
              "seed": seed}
        fx.update(record(Evaluator, scores, target, ignore))
        path = os.path.join(GOLD, name + ".pt")
        torch.save(fx, path)
        print(name, os.path.getsize(path), "bytes", {k: v.tolist() for k, v in fx.items() if k.startswith("area_")})


if __name__ == "__main__":
    main()
