#!/usr/bin/env python
"""Time the LSegNet training step WITH the arch_option 1/2 head blocks (lseg_config.flags bit 4, csrc/head_train.hip) next to the plain
arch_option 0 step: same backbone, crop, per-GPU batch and K shared labels, in one process (tools; bench.py is not involved).  Each step:
train-mode forward (no full-resolution logits) + fused cross-entropy + backward + fused SGD.  The engines run one after the other (each
is closed before the next is built).  Prints one JSON line.

    python tools/head_train_bench.py [--batch 8] [--size 480] [--depth 2] [--steps 5] [--warmup 2]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "lang-seg_amd"))
sys.path.insert(0, ROOT)
import torch                                                                      # noqa: E402
from lseg_hip.config import get_config                                            # noqa: E402
from lseg_hip.engine import HipEngine                                             # noqa: E402
from lseg_hip.synth import synthetic_state_dict, synthetic_tokens, synthetic_images, read_labels   # noqa: E402


def run(cfg, x, tok, target, steps, warmup):
    B, _, H, W = x.shape
    sd = {k: v.cuda() for k, v in synthetic_state_dict(cfg, seed=0).items()}
    eng = HipEngine(cfg, H, W, max_batch=B, max_labels=tok.shape[0], head_block_training=cfg.arch_option in (1, 2))
    eng.load_state_dict(sd)
    eng.set_tokens(tok)
    eng.enable_training(sd)
    ms = []
    for s in range(warmup + steps):
        e0, e1, e2, e3 = (torch.cuda.Event(enable_timing=True) for _ in range(4))
        e0.record()
        eng.forward(x, want_logits=False)
        e1.record()
        loss = eng.backward(target=target, ignore_index=-1)
        e2.record()
        eng.sgd_step(1e-4, 1e-3, 0.9, 1e-4)
        e3.record()
        torch.cuda.synchronize()
        if s >= warmup:
            ms.append((e0.elapsed_time(e3), e0.elapsed_time(e1), e1.elapsed_time(e2), e2.elapsed_time(e3)))
    eng.close()
    del sd
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    med = lambda i: sorted(m[i] for m in ms)[len(ms) // 2]
    return {"step_ms": round(med(0), 2), "forward_ms": round(med(1), 2), "backward_ms": round(med(2), 2), "sgd_ms": round(med(3), 2),
            "step_ms_all": [round(m[0], 2) for m in ms], "loss": float(loss)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--backbone", default="clip_vitl16_384")
    ap.add_argument("--size", type=int, default=480)
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--labels", type=int, default=150)
    ap.add_argument("--depth", type=int, default=2)
    ap.add_argument("--activation", default="lrelu")
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    a = ap.parse_args()
    B, S = a.batch, a.size
    x = synthetic_images(B, S, S, seed=0).cuda()
    g = torch.Generator().manual_seed(1)
    labels = read_labels(os.path.join(ROOT, "lang-seg_amd", "label_files", "ade20k_objectInfo150.txt"))[: a.labels]
    t = torch.randint(0, len(labels), (B, S, S), generator=g)
    t[torch.rand(t.shape, generator=g) < 0.2] = -1
    t = t.cuda()
    t0 = time.perf_counter()
    out = {"tool": "head_train_bench", "backbone": a.backbone, "size": S, "batch": B, "labels": len(labels), "steps": a.steps,
           "warmup": a.warmup, "activation": a.activation}
    for arch in (0, 1, 2):
        cfg = get_config(a.backbone, arch_option=arch, block_depth=a.depth if arch else 0, activation=a.activation)
        tok = synthetic_tokens(labels, cfg.text.vocab, cfg.text.ctx)
        out[f"arch{arch}" + (f"_depth{a.depth}" if arch else "")] = run(cfg, x, tok, t, a.steps, a.warmup)
    base = out["arch0"]["step_ms"]
    for arch in (1, 2):
        r = out[f"arch{arch}_depth{a.depth}"]
        r["over_arch0_ms"] = round(r["step_ms"] - base, 2)
    out["wall_s"] = round(time.perf_counter() - t0, 1)
    out["device"] = torch.cuda.get_device_name(0)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
