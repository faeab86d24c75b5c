#!/usr/bin/env python
"""Time the ZERO-SHOT training step (LSegNetZS: per-image label pairs, G = 2) next to the LSegNet step with K = 150 shared labels, same
backbone, crop and per-GPU batch, in one process (tools; bench.py is not involved).  Each step: train-mode forward (no full-resolution
logits) + fused cross-entropy + backward + fused SGD, as LSegmentationModule(ZS).training_step -> loss.backward() -> optimizer.step()
drive it.  The engines run one after the other (the first is closed before the second is built).  Prints one JSON line.

    python tools/zs_train_bench.py [--batch 8] [--size 480] [--steps 5] [--warmup 2]
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


def run(cfg, sd, x, tok, target, group, ignore, steps, warmup):
    B, _, H, W = x.shape
    eng = HipEngine(cfg, H, W, max_batch=B, max_labels=tok.shape[0])
    eng.load_state_dict(sd)
    eng.set_tokens(tok, labels_per_image=group)
    eng.enable_training(sd)
    ms = []
    for s in range(warmup + steps):
        e0, e1, e2, e3 = (torch.cuda.Event(enable_timing=True) for _ in range(4))
        e0.record()
        eng.forward(x, want_logits=False)
        e1.record()
        loss = eng.backward(target=target, ignore_index=ignore)
        e2.record()
        eng.sgd_step(1e-4, 1e-3, 0.9, 1e-4)
        e3.record()
        torch.cuda.synchronize()
        if s >= warmup:
            ms.append((e0.elapsed_time(e3), e0.elapsed_time(e1), e1.elapsed_time(e2), e2.elapsed_time(e3)))
    eng.close()
    torch.cuda.synchronize()
    med = lambda i: sorted(m[i] for m in ms)[len(ms) // 2]
    return {"step_ms": round(med(0), 2), "forward_ms": round(med(1), 2), "backward_ms": round(med(2), 2), "sgd_ms": round(med(3), 2),
            "step_ms_all": [round(m[0], 2) for m in ms], "loss": float(loss)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--backbone", default="clip_vitl16_384")
    ap.add_argument("--size", type=int, default=480)
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--labels", type=int, default=150)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    a = ap.parse_args()
    cfg = get_config(a.backbone)
    sd = {k: v.cuda() for k, v in synthetic_state_dict(cfg, seed=0).items()}
    B, S = a.batch, a.size
    x = synthetic_images(B, S, S, seed=0).cuda()
    g = torch.Generator().manual_seed(1)
    # zero-shot: ['others', class] per image, 0/1 masks, torch's default ignore_index (LSegmentationModuleZS.criterion)
    fss = read_labels(os.path.join(ROOT, "lang-seg_amd", "label_files", "fewshot_fss.txt"), skip_header=False)
    ids = [(7 * i + 3) % len(fss) for i in range(B)]
    tok_zs = torch.cat([synthetic_tokens(["others", fss[c]], cfg.text.vocab, cfg.text.ctx) for c in ids], 0)
    t_zs = torch.randint(0, 2, (B, S, S), generator=g).cuda()
    # LSegNet: K shared ADE20K labels, 20 % ignored pixels (lsegmentation_module.py, ignore_index -1)
    labels = read_labels(os.path.join(ROOT, "lang-seg_amd", "label_files", "ade20k_objectInfo150.txt"))[: a.labels]
    tok = synthetic_tokens(labels, cfg.text.vocab, cfg.text.ctx)
    t = torch.randint(0, len(labels), (B, S, S), generator=g)
    t[torch.rand(t.shape, generator=g) < 0.2] = -1
    t = t.cuda()
    t0 = time.perf_counter()
    zs = run(cfg, sd, x, tok_zs, t_zs, 2, -100, a.steps, a.warmup)
    shared = run(cfg, sd, x, tok, t, 0, -1, a.steps, a.warmup)
    out = {"tool": "zs_train_bench", "backbone": a.backbone, "size": S, "batch": B, "steps": a.steps, "warmup": a.warmup,
           "zero_shot_G2": zs, f"lsegnet_K{len(labels)}": shared,
           "zs_over_shared": round(zs["step_ms"] / shared["step_ms"], 4), "wall_s": round(time.perf_counter() - t0, 1),
           "device": torch.cuda.get_device_name(0)}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
