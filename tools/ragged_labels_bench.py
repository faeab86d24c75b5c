#!/usr/bin/env python3
"""Open-vocabulary batches: 36 images, each with its OWN list of candidate labels, of its own length -- ms for the masks of all 36 on
ViT-L/16 at 480 x 480, fp16 operands, the two ways there are:

  (a) one ragged forward      set_tokens(all lists, group_sizes=counts) + ONE forward_labels at B = 36 (lseg_set_text_groups: the streamed
                              kernel correlates every image with its own rows, csrc/corr_argmax.hip RAGGED)
  (b) 36 forwards at B = 1    set_tokens(list b) + forward_labels(image b), 36 times: the only route without ragged groups

The counts come from random.Random(SEED).randint(2, 150) and are written into the output.  Text cache OFF in both legs, and set_tokens
inside the timed region: a server sees new lists with every request, so the text tower runs in every forward ((a) encodes all
sum(counts) labels in one go, (b) one list at a time).  Timing: warm-up, then the median of REPEATS medians-of-ITERS, device events
around one whole leg, both legs in one process.

    python tools/ragged_labels_bench.py [--out profiles/ragged_labels.txt]
"""
import argparse
import os
import random
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

WARMUP, ITERS, REPEATS = 2, 3, 3
SEED, B, SIZE = 0, 36, 480


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ragged_labels.txt"))
    ap.add_argument("--images", type=int, default=B)
    ap.add_argument("--size", type=int, default=SIZE)
    a = ap.parse_args()
    torch.cuda.set_device(0)
    rng = random.Random(SEED)
    counts = [rng.randint(2, 150) for _ in range(a.images)]
    K = sum(counts)
    cfg = get_config("clip_vitl16_384")
    eng = HipEngine(cfg, a.size, a.size, max_batch=a.images, max_labels=K, image_dtype="fp16")
    eng.load_state_dict(synthetic_state_dict(cfg, seed=0))
    lists = [[f"thing number {i} of image {b}" for i in range(k)] for b, k in enumerate(counts)]
    toks = [synthetic_tokens(ls, cfg.text.vocab, cfg.text.ctx) for ls in lists]
    tok_all = torch.cat(toks)
    x = synthetic_images(a.images, a.size, a.size, seed=1).cuda()
    xs = [x[b:b + 1].contiguous() for b in range(a.images)]

    def ragged():
        eng.set_tokens(tok_all, group_sizes=counts)
        return eng.forward_labels(x)

    def one_by_one():
        out = []
        for b in range(a.images):
            eng.set_tokens(toks[b])
            out.append(eng.forward_labels(xs[b]))
        return torch.cat(out)

    lines = ["# tools/ragged_labels_bench.py -- ViT-L/16, %d x %d, fp16 operands, %d images, one label list each, text cache off, set_tokens "
             "timed; ms = median of %d medians of %d (min .. max of the medians)" % (a.size, a.size, a.images, REPEATS, ITERS),
             "# counts (random.Random(%d).randint(2, 150)), %d labels in all: %s" % (SEED, K, " ".join(str(k) for k in counts)),
             "# %-44s %10s %22s %12s" % ("leg", "ms", "(min .. max)", "images/s")]
    res = {}
    for name, fn in (("(a) one ragged forward_labels, B = %d" % a.images, ragged), ("(b) %d forward_labels at B = 1" % a.images, one_by_one)):
        ms, lo, hi = timed(fn)
        res[name] = fn()
        lines.append("  %-44s %10.3f %22s %12.1f" % (name, ms, "(%.3f .. %.3f)" % (lo, hi), a.images * 1e3 / ms))
        print(lines[-1], flush=True)
    ra, rb = res.values()
    torch.cuda.synchronize()
    lines.append("  labels differing between (a) and (b): %d of %d pixels (the B = %d and B = 1 towers take different GEMM plans)"
                 % ((ra != rb).sum().item(), ra.numel(), a.images))
    print(lines[-1], flush=True)
    eng.close()
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()
