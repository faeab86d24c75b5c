#!/usr/bin/env python3
"""Masks for large label sets: ms per forward and peak device memory of the two ways to a [B,480,480] mask on ViT-L/16, fp16 operands.

  (a) logits + torch.argmax   lseg_forward into a [B,K,480,480] fp32 buffer, then torch.argmax(1) -- the only way to a K > 256 mask
                              before lseg_forward_labels
  (a') uint8 masks            lseg_forward(dev_logits_out = NULL, dev_argmax_out): the K <= 256 product
  (b) forward_labels          lseg_forward_labels: streamed-panel correlation + arg-max (csrc/corr_argmax.hip), int16

K in {150, 256, 1000}, B in {1, 4}; text features cached (the text tower is not what is compared).  Timing: warm-up, then the median of
REPEATS medians-of-ITERS (device events around ITERS back-to-back forwards), all variants in one process.  Peak memory: torch's allocator
peak over one call (the engine's own buffers are the same for every variant and are not counted).

    python tools/large_k_bench.py [--out profiles/large_k_masks.txt]
"""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "lang-seg_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)
os.environ.setdefault("LSEG_SYNTHETIC_TOKENS", "1")

import torch                                                              # noqa: E402
from lseg_hip.config import get_config                                    # noqa: E402
from lseg_hip.engine import HipEngine                                     # noqa: E402
from lseg_hip.synth import synthetic_state_dict, synthetic_tokens, synthetic_images   # noqa: E402

WARMUP, ITERS, REPEATS = 3, 5, 3


def timed(fn):
    for _ in range(WARMUP):
        fn()
    torch.cuda.synchronize()
    meds = []
    for _ in range(REPEATS):
        ts = []
        for _ in range(ITERS):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            ts.append(e0.elapsed_time(e1))
        meds.append(statistics.median(ts))
    return statistics.median(meds), min(meds), max(meds)


def peak(fn):
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    r = fn()
    torch.cuda.synchronize()
    p = torch.cuda.max_memory_allocated() - base
    del r
    return p


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "large_k_masks.txt"))
    ap.add_argument("--ks", default="150,256,1000")
    ap.add_argument("--bs", default="1,4")
    a = ap.parse_args()
    torch.cuda.set_device(0)
    cfg = get_config("clip_vitl16_384")
    sd = synthetic_state_dict(cfg, seed=0)
    lines = ["# tools/large_k_bench.py -- ViT-L/16, 480 x 480, fp16 operands, text features cached; ms = median of %d medians of %d "
             "(min .. max of the medians); peak = torch allocator peak over one call" % (REPEATS, ITERS),
             "# %-5s %-3s %-28s %10s %18s %12s" % ("K", "B", "variant", "ms", "(min .. max)", "peak MB")]
    for K in [int(k) for k in a.ks.split(",")]:
        eng = HipEngine(cfg, 480, 480, max_batch=4, max_labels=K, image_dtype="fp16")
        eng.load_state_dict(sd)
        eng.set_tokens(synthetic_tokens([f"thing number {i}" for i in range(K)], cfg.text.vocab, cfg.text.ctx))
        eng.set_text_cache(True)
        for B in [int(b) for b in a.bs.split(",")]:
            x = synthetic_images(B, 480, 480, seed=1).cuda()
            variants = [("logits + torch.argmax", lambda: eng.forward(x).argmax(1))]
            if K <= 256:
                variants.append(("uint8 masks (lseg_forward)", lambda: eng.forward(x, want_logits=False, want_argmax=True)))
            variants.append(("forward_labels (int16)", lambda: eng.forward_labels(x)))
            variants.append(("forward_labels + score", lambda: eng.forward_labels(x, want_score=True)))
            ref = None
            for name, fn in variants:
                ms, lo, hi = timed(fn)
                pk = peak(fn)
                lines.append("  %-5d %-3d %-28s %10.3f %18s %12.1f" % (K, B, name, ms, "(%.3f .. %.3f)" % (lo, hi), pk / 2 ** 20))
                print(lines[-1], flush=True)
                r = fn()
                r = (r[0] if isinstance(r, tuple) else r).long()
                if ref is None:
                    ref = r
                else:
                    lines.append("        labels differing from logits + torch.argmax: %d of %d pixels" % ((r != ref).sum().item(), r.numel()))
                    print(lines[-1], flush=True)
                del r
            del ref
        eng.close()
        del eng
        torch.cuda.empty_cache()
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()
