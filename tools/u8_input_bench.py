#!/usr/bin/env python
"""Time decoded uint8 images in (HipEngine.set_input_u8: ToTensor + Normalize fused into the first stage) against what a caller did
before it existed: the same uint8 tensor through torch permute / float / div / sub / div on the GPU, then the fp32 entry.
(tools; bench.py is not involved.)  ViT-L/16 at 480 x 480, K = 150 labels, text cache on, masks out (forward_labels), B = 36 and B = 1;
then one 512 x 683 image through BatchedMultiEval.forward both ways (the torch route normalises once and hands the float image over).
Synthetic weights and images, seeded.  The two routes alternate call by call in one process; every call is timed with device events
around work that ends in a synchronise; medians and the spread (min .. max) over the timed calls.  Prints one JSON line.

    python tools/u8_input_bench.py [--steps 20] [--warmup 3] [--eval-steps 3] [--backbone clip_vitl16_384] [--size 480]

Note on route (b): torch's GPU kernel for `x.div(255)` multiplies by the reciprocal, so its tensor differs from the host transform's
(and from the uint8 path's) in the last bit of some values; the timing is what is compared here, the bits are tests/test_gpu_input_u8.py's.
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "lang-seg_amd"))
sys.path.insert(0, ROOT)
os.environ.setdefault("LSEG_SYNTHETIC_TOKENS", "1")     # synthetic weights: stand-in token ids (lseg_hip/tokenizer.py)
import torch                                                                   # noqa: E402
from lseg_hip.config import get_config                                            # noqa: E402
from lseg_hip.engine import HipEngine                                             # noqa: E402
from lseg_hip.evaluator import BatchedMultiEval, ModuleSurface                    # noqa: E402
from lseg_hip.synth import synthetic_state_dict, synthetic_tokens                 # noqa: E402

MEAN, STD = (0.5, 0.5, 0.5), (0.5, 0.5, 0.5)


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1)


def summary(ms):
    s = sorted(ms)
    return {"median_ms": round(s[len(s) // 2], 3), "min_ms": round(s[0], 3), "max_ms": round(s[-1], 3), "calls": len(s)}


def torch_normalize(u8, mean, std):
    """what a caller does on the GPU in front of the fp32 entry: three elementwise passes and a layout change"""
    return u8.permute(0, 3, 1, 2).float().div(255).sub(mean).div(std).contiguous()


def alternate(route_a, route_b, steps, warmup):
    a, b = [], []
    for s in range(warmup + steps):
        ta, tb = timed(route_a), timed(route_b)
        if s >= warmup:
            a.append(ta)
            b.append(tb)
    return summary(a), summary(b)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--eval-steps", type=int, default=3)
    ap.add_argument("--backbone", default="clip_vitl16_384")
    ap.add_argument("--size", type=int, default=480)
    ap.add_argument("--labels", type=int, default=150)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("u8_input_bench needs a GPU: a timing taken anywhere else says nothing")
    cfg = get_config(a.backbone)
    sd = {k: v.cuda() for k, v in synthetic_state_dict(cfg, seed=0).items()}
    names = [f"label{i}" for i in range(a.labels)]
    tok = synthetic_tokens(names, cfg.text.vocab, cfg.text.ctx)
    mean = torch.tensor(MEAN, device="cuda").view(1, 3, 1, 1)
    std = torch.tensor(STD, device="cuda").view(1, 3, 1, 1)
    g = torch.Generator().manual_seed(0)
    out = {"backbone": a.backbone, "size": a.size, "labels": a.labels, "output": "forward_labels (int16 masks)"}
    try:
        out["build"] = open(os.path.join(ROOT, "lang-seg_amd", "lseg_hip", "_build_id.txt")).read().strip()
    except OSError:
        out["build"] = "unknown"
    for B in (36, 1):
        u8 = torch.randint(0, 256, (B, a.size, a.size, 3), generator=g, dtype=torch.uint8).cuda()
        eng = HipEngine(cfg, a.size, a.size, max_batch=B, max_labels=a.labels)
        eng.load_state_dict(sd)
        eng.set_tokens(tok)
        eng.set_text_cache(True)

        def route_u8():
            eng.set_input_u8(True, MEAN, STD)
            eng.forward_labels(u8)

        def route_torch():
            eng.set_input_u8(False)
            eng.forward_labels(torch_normalize(u8, mean, std))

        ru, rt = alternate(route_u8, route_torch, a.steps, a.warmup)
        norm_only = summary([timed(lambda: torch_normalize(u8, mean, std)) for _ in range(a.warmup + a.steps)][a.warmup:])
        out[f"B{B}"] = {"uint8_in": ru, "torch_normalize_then_fp32": rt, "torch_normalize_alone": norm_only,
                        "images_per_s_uint8": round(1000.0 * B / ru["median_ms"], 1), "images_per_s_torch": round(1000.0 * B / rt["median_ms"], 1)}
        print(f"B={B}: {json.dumps(out[f'B{B}'])}", file=sys.stderr)
        eng.close()
        del eng, u8
        torch.cuda.synchronize()
    # the multi-scale evaluator on one 512 x 683 image, both ways
    from modules.models.lseg_net import LSegNet
    net = LSegNet(labels=names, backbone=a.backbone, features=cfg.features, arch_option=0, block_depth=0, activation="lrelu")
    net.load_state_dict({k: v for k, v in synthetic_state_dict(cfg, seed=0).items()}, strict=False)
    net = net.cuda().eval()
    ev = BatchedMultiEval(ModuleSurface(net, crop_size=a.size, base_size=520, mean=MEAN, std=STD), a.labels, lowres=True)
    img = torch.randint(0, 256, (512, 683, 3), generator=g, dtype=torch.uint8).cuda()
    eu, et = alternate(lambda: ev.forward(img), lambda: ev.forward(torch_normalize(img.unsqueeze(0), mean, std)), a.eval_steps, 1)
    out["multi_eval_512x683"] = {"uint8_in": eu, "torch_normalize_then_fp32": et, "scales": ev.scales, "flip": ev.flip, "lowres": True}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
