"""Multi-scale masks over label panels, timed and weighed against the score tensor: BatchedMultiEval.forward_labels -- the image tower once
per crop (hold_features), the label set in panels over the held features (score_held), lseg_op_eval_merge_labels per panel -- beside
BatchedMultiEval(lowres=True).forward + torch.max, the only route to the masks before it.  Workload of tools/eval_lowres_bench.py:
ViT-L/16, crop 480 / base 520, one 512 x 683 image, 6 scales + flip, synthetic weights; K = 150 and K = 1000 through evaluate_random.
The paths run in ONE process, alternating, `--repeats` times; the table gives the median ms per image, the range, and
torch.cuda.max_memory_allocated of one call above the resident tensors (the engine's own workspace is allocated outside torch's allocator
and is the same for every path: its label planes are sized max_batch x max_labels whichever path runs).  Beside each measured peak of
forward_labels stands the bound computed from the layout: held features + panel x (largest forward group's low-resolution logits +
score tensor + largest scale map) + the state planes.

    python tools/eval_labels_bench.py [--out profiles/eval_labels.txt]
"""
import argparse
import os
import statistics
import sys
import time
import warnings

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "lang-seg_amd")]
os.environ.setdefault("LSEG_SYNTHETIC_TOKENS", "1")

import torch                                             # noqa: E402

from lseg_hip.config import get_config                   # noqa: E402
from lseg_hip.evaluator import BatchedMultiEval, ModuleSurface, plan_schedule, scale_geometry   # noqa: E402
from lseg_hip.synth import synthetic_state_dict, synthetic_images   # noqa: E402

SCALES = (0.5, 0.75, 1.0, 1.25, 1.5, 1.75)


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def peak_of(fn):
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    fn()
    torch.cuda.synchronize()
    return torch.cuda.max_memory_allocated() - base


def computed_bound(h, w, crop, base, panel, K, max_batch, out_c=512):
    """bytes: held features of every crop + panel x (low-resolution logits of the largest forward group + [rows,h,w] scores + largest
    scale map) + the five state planes; the crops of the largest step are alive beside it while the towers run"""
    geo = [scale_geometry(h, w, s, base, crop) for s in SCALES]
    steps, largest = plan_schedule(geo, True, 192, max_batch)
    crops = 2 * sum(g.n_box for g in geo)
    held = crops * ((crop // 4 + 2) ** 2 * out_c * 2 + (crop // 2) ** 2 * 4)
    rows = min(panel, K)
    group = max(sum(2 * geo[i].n_box for i in st.scales) if st.windows is None else max(2 * nb for _, nb in st.windows) for st in steps)
    per_panel = rows * (group * (crop // 2) ** 2 + h * w + max(g.height * g.width for g in geo)) * 4
    state = h * w * (2 + 4 + 2 + 4 + 4)
    return held, per_panel, state, crops


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--backbone", default="clip_vitl16_384")
    ap.add_argument("--crop", type=int, default=480)
    ap.add_argument("--base", type=int, default=520)
    ap.add_argument("--image", type=int, nargs=2, default=[512, 683])
    ap.add_argument("--labels", type=int, nargs="+", default=[150, 1000])
    ap.add_argument("--panels", type=int, nargs="+", default=[64, 160])
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    warnings.simplefilter("ignore")
    from modules.models.lseg_net import LSegNet
    cfg = get_config(args.backbone)
    net = LSegNet(labels=["wall", "sky"], backbone=args.backbone, features=cfg.features, arch_option=0, block_depth=0, activation="lrelu")
    net.load_state_dict(synthetic_state_dict(cfg, seed=0))
    mod = ModuleSurface(net.cuda().eval(), crop_size=args.crop, base_size=args.base)
    h, w = args.image
    img = synthetic_images(1, h, w, seed=9).cuda()
    ev = BatchedMultiEval(mod, 2, flip=True, scales=SCALES, lowres=True)
    lines = [f"multi-scale masks, {args.backbone} crop {args.crop} / base {args.base}, one {h}x{w} image, scales {SCALES} + flip, synthetic weights, "
             f"image_dtype {net.image_dtype}, max_batch {ev.max_batch}",
             f"median of {args.repeats} calls per path, the paths alternating in one process; ms per image (min .. max); peak = "
             "torch.cuda.max_memory_allocated of one call above the resident tensors", ""]
    with torch.no_grad():
        for K in args.labels:
            labels = [f"thing number {i}" for i in range(K)]
            paths = {"forward(lowres) + torch.max": lambda: torch.max(ev(img, labels), 1)}
            for p in args.panels:
                paths[f"forward_labels panel {p}"] = lambda p=p: ev.forward_labels(img, labels, panel=p)
                paths[f"forward_labels panel {p} +conf"] = lambda p=p: ev.forward_labels(img, labels, confidence=True, panel=p)
            lines.append(f"K = {K}")
            ok, t, peak = {}, {}, {}
            for name, fn in paths.items():                              # engines, text features, allocator pools; a path that cannot run says so
                try:
                    fn()
                    torch.cuda.synchronize()
                    ok[name], t[name] = True, []
                except (RuntimeError, torch.cuda.OutOfMemoryError) as e:
                    ok[name] = False
                    lines.append(f"  {name:34s} failed: {type(e).__name__}: {str(e).splitlines()[0][:160]}")
                torch.cuda.empty_cache()
            want = torch.max(ev(img, labels), 1) if ok["forward(lowres) + torch.max"] else None
            for _ in range(args.repeats):
                for name, fn in paths.items():
                    if ok[name]:
                        t[name].append(timed(fn))
            for name, fn in paths.items():
                if ok[name]:
                    torch.cuda.empty_cache()
                    peak[name] = peak_of(fn)
            for name in paths:
                if not ok[name]:
                    continue
                med = statistics.median(t[name])
                line = f"  {name:34s} {med:9.2f} ms ({min(t[name]):.2f} .. {max(t[name]):.2f})   peak {peak[name] / 1e6:9.1f} MB"
                if name.startswith("forward_labels"):
                    p = int(name.split()[2])
                    held, per_panel, state, crops = computed_bound(h, w, args.crop, args.base, p, K, ev.max_batch)
                    line += (f"   computed {(held + per_panel + state) / 1e6:8.1f} MB = held {held / 1e6:.1f} ({crops} crops) + panel "
                             f"{per_panel / 1e6:.1f} + state {state / 1e6:.1f}")
                lines.append(line)
            if want is not None:
                lab, score = ev.forward_labels(img, labels, panel=args.panels[0])
                same = torch.equal(lab.long(), want[1][0]) and torch.equal(score, want[0][0])
                lines.append(f"  labels and scores equal torch.max of the score tensor bit for bit: {same}"
                             + ("" if K > 157 else "  (K <= 157: the score tensor's scale plane comes from the fused kernel's dot products, "
                                                   f"{int((lab.long() != want[1][0]).sum())} of {lab.numel()} labels differ)"))
                del want
            lines.append("")
            torch.cuda.empty_cache()
    text = "\n".join(lines)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
