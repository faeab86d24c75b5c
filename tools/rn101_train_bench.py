"""Step time and device memory of the LSegRNNetZS decoder-training step (HipEngine(train_resnet_decoder=True): ResNet-101 tower in train()
mode, backward of scratch.* only) at 480 x 480, B = 8 and B = 20 (the reference's few-shot batch size), beside the ViT-L/16
frozen-encoder zero-shot step in the same process.  Forward, backward and optimizer step are timed separately with HIP events; the
memory figure is the device's used memory with the engine alive minus the memory used before it was built.

    python tools/rn101_train_bench.py [--steps 10] [--warmup 3] [--out profiles/rn101_train_decoder.txt]
"""
import argparse
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "lang-seg_amd"))
os.environ.setdefault("LSEG_SYNTHETIC_TOKENS", "1")

from lseg_hip.config import get_config                                            # noqa: E402
from lseg_hip.engine import HipEngine                                             # noqa: E402
from lseg_hip.synth import synthetic_images, synthetic_state_dict, synthetic_tokens   # noqa: E402


def used_mib():
    free, total = torch.cuda.mem_get_info()
    return (total - free) / 2 ** 20


def bench(kind, B, steps, warmup, H=480, W=480):
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    base = used_mib()
    cfg = get_config("clip_resnet101" if kind == "rn101" else "clip_vitl16_384")
    sd = {k: v.cuda() for k, v in synthetic_state_dict(cfg, seed=1).items()}
    tok = torch.cat([synthetic_tokens(["others", f"class{c}"], cfg.text.vocab, cfg.text.ctx) for c in range(B)], 0)
    eng = HipEngine(cfg, H, W, max_batch=B, max_labels=2 * B, train_resnet_decoder=(kind == "rn101"))
    eng.load_state_dict(sd)
    eng.set_tokens(tok, labels_per_image=2)
    eng.enable_training(sd, freeze_encoder=(kind != "rn101"))
    x = synthetic_images(B, H, W, seed=1).cuda()
    target = torch.randint(0, 2, (B, H, W), generator=torch.Generator().manual_seed(1)).cuda()
    ev = [[torch.cuda.Event(enable_timing=True) for _ in range(4)] for _ in range(steps)]
    for i in range(warmup + steps):
        e = ev[i - warmup] if i >= warmup else None
        if e: e[0].record()
        eng.forward(x, want_logits=False)
        if e: e[1].record()
        eng.backward(target=target, ignore_index=-100)
        if e: e[2].record()
        eng.sgd_step(1e-4, 1e-3, 0.9, 1e-4)
        if e: e[3].record()
    torch.cuda.synchronize()
    peak = used_mib() - base
    med = lambda v: sorted(v)[len(v) // 2]                   # noqa: E731
    fwd, bwd, opt = (med([e[j].elapsed_time(e[j + 1]) for e in ev]) for j in range(3))
    eng.close()
    del sd
    name = "LSegRNNetZS decoder step (RN101 tower in train mode)" if kind == "rn101" else "LSegNetZS ViT-L/16 frozen-encoder step"
    return (f"{name:56s} B={B:2d} {H}x{W}: forward {fwd:7.2f} ms  backward {bwd:7.2f} ms  optimizer {opt:5.2f} ms  "
            f"step {fwd + bwd + opt:7.2f} ms  {B / (fwd + bwd + opt) * 1e3:6.1f} img/s  device memory {peak / 1024:6.2f} GiB")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    lines = [f"{torch.cuda.get_device_name(0)}; median of {a.steps} steps after {a.warmup} warm-up steps; synthetic weights, per-image label pairs"]
    for B in (8, 20):
        for kind in ("rn101", "vitl16_frozen"):
            lines.append(bench(kind, B, a.steps, a.warmup))
            print(lines[-1], flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
