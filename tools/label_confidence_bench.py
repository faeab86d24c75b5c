#!/usr/bin/env python3
"""Label confidence without logits: ms per forward and peak device memory of the ways to (label, score, runner-up, log-sum-exp) per pixel
on ViT-L/16, 480 x 480, fp16 operands -- a sibling of tools/large_k_bench.py (same timing and peak-memory method).

  (a) forward_labels + score     lseg_forward_labels: the arg-max alone (what the confidence variant adds its state to)
  (b) forward_labels_conf        lseg_forward_labels_conf: streamed-panel correlation with the running top-2 + log-sum-exp
  (c) logits + topk + logsumexp  lseg_forward into a [B,K,480,480] fp32 buffer, then torch.topk(pred, 2, 1) and torch.logsumexp(pred, 1)

K in {150, 1000}, B = 4; text features cached.  Also prints how far (b) is from (c): labels differing, max |lse difference|.

    python tools/label_confidence_bench.py [--out profiles/label_confidence.txt]
"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "lang-seg_amd"), os.path.join(ROOT, "tools")):
    if p not in sys.path:
        sys.path.insert(0, p)
os.environ.setdefault("LSEG_SYNTHETIC_TOKENS", "1")

import torch                                                              # noqa: E402
from large_k_bench import timed, peak, WARMUP, ITERS, REPEATS             # noqa: E402
from lseg_hip.config import get_config                                    # noqa: E402
from lseg_hip.engine import HipEngine                                     # noqa: E402
from lseg_hip.synth import synthetic_state_dict, synthetic_tokens, synthetic_images   # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "label_confidence.txt"))
    ap.add_argument("--ks", default="150,1000")
    ap.add_argument("--bs", default="4")
    a = ap.parse_args()
    torch.cuda.set_device(0)
    cfg = get_config("clip_vitl16_384")
    sd = synthetic_state_dict(cfg, seed=0)
    lines = ["# tools/label_confidence_bench.py -- ViT-L/16, 480 x 480, fp16 operands, text features cached; ms = median of %d medians of %d "
             "(min .. max of the medians); peak = torch allocator peak over one call" % (REPEATS, ITERS),
             "# %-5s %-3s %-30s %10s %18s %12s" % ("K", "B", "variant", "ms", "(min .. max)", "peak MB")]

    def via_logits(eng, x):
        out = eng.forward(x)
        top = torch.topk(out, 2, 1)
        return top.indices[:, 0], top.values[:, 0], top.indices[:, 1], top.values[:, 1], torch.logsumexp(out, 1)

    for K in [int(k) for k in a.ks.split(",")]:
        eng = HipEngine(cfg, 480, 480, max_batch=4, max_labels=K, image_dtype="fp16")
        eng.load_state_dict(sd)
        eng.set_tokens(synthetic_tokens([f"thing number {i}" for i in range(K)], cfg.text.vocab, cfg.text.ctx))
        eng.set_text_cache(True)
        for B in [int(b) for b in a.bs.split(",")]:
            x = synthetic_images(B, 480, 480, seed=1).cuda()
            variants = [("forward_labels + score", lambda: eng.forward_labels(x, want_score=True)),
                        ("forward_labels_conf", lambda: eng.forward_labels_conf(x)),
                        ("logits + topk + logsumexp", lambda: via_logits(eng, x))]
            for name, fn in variants:
                ms, lo, hi = timed(fn)
                pk = peak(fn)
                lines.append("  %-5d %-3d %-30s %10.3f %18s %12.1f" % (K, B, name, ms, "(%.3f .. %.3f)" % (lo, hi), pk / 2 ** 20))
                print(lines[-1], flush=True)
            r = eng.forward_labels_conf(x)
            l1, s1, l2, s2, lse = via_logits(eng, x)
            lines.append("        vs logits + topk + logsumexp: label differs at %d, label2 at %d of %d pixels (torch.topk breaks ties its own "
                         "way); max |score diff| %.3e, |score2 diff| %.3e, |lse diff| %.3e"
                         % ((r["label"].long() != l1).sum().item(), (r["label2"].long() != l2).sum().item(), l1.numel(),
                            (r["score"] - s1).abs().max().item(), (r["score2"] - s2).abs().max().item(), (r["lse"] - lse).abs().max().item()))
            print(lines[-1], flush=True)
            del r, l1, s1, l2, s2, lse
        eng.close()
        del eng
        torch.cuda.empty_cache()
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()
