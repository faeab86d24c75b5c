"""The multi-scale evaluator where ONE scale has more crops than max_stack: ViT-L/16, crop 480 / base 2048 (the reference's --base_size /
--crop_size are user flags), one synthetic 1024 x 2048 image, 6 scales + flip, K = 150, synthetic weights.  At scale 1.75 the grid is
11 x 6 boxes = 132 crops with their mirrored twins, 18 GB of full-resolution logits as one stack; BatchedMultiEval runs such a scale in
windows of whole boxes (lseg_op_eval_accumulate_window + lseg_op_eval_finalize).  Prints the crops per scale, the milliseconds per image
(median of --repeats, min .. max) and torch.cuda.max_memory_allocated of one call above the resident tensors, next to the bound
max_stack x per-crop logits + the maps, for lowres False and True.  An out-of-memory error of a path is recorded, not raised.

--tree DIR imports lseg_hip / modules from another checkout (its lang-seg_amd directory is DIR/lang-seg_amd), so the same tool measures
the commit before this one; LSEG_HIP_LIB chooses the library as everywhere else.

    python tools/eval_window_bench.py [--out profiles/eval_window.txt] [--tree DIR] [--max-stack N]
"""
import argparse
import os
import statistics
import sys
import time
import warnings

ap = argparse.ArgumentParser()
ap.add_argument("--tree", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
ap.add_argument("--backbone", default="clip_vitl16_384")
ap.add_argument("--crop", type=int, default=480)
ap.add_argument("--base", type=int, default=2048)
ap.add_argument("--image", type=int, nargs=2, default=[1024, 2048])
ap.add_argument("--labels", type=int, default=150)
ap.add_argument("--max-stack", type=int, default=None, help="set the evaluator's max_stack attribute (default: the evaluator's own 48 / 192)")
ap.add_argument("--max-batch", type=int, default=36)
ap.add_argument("--repeats", type=int, default=3)
ap.add_argument("--lowres", choices=["both", "0", "1"], default="both")
ap.add_argument("--out", default=None)
args = ap.parse_args()

ROOT = os.path.abspath(args.tree)
sys.path[:0] = [ROOT, os.path.join(ROOT, "lang-seg_amd")]
os.environ.setdefault("LSEG_SYNTHETIC_TOKENS", "1")

import torch                                             # noqa: E402

from lseg_hip.config import get_config                   # noqa: E402
from lseg_hip.evaluator import BatchedMultiEval, ModuleSurface, scale_geometry   # noqa: E402
from lseg_hip.synth import synthetic_state_dict, synthetic_images, read_labels   # noqa: E402

SCALES = (0.5, 0.75, 1.0, 1.25, 1.5, 1.75)


def one_image(ev, img):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = ev(img)
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, out


def main():
    warnings.simplefilter("ignore")
    from modules.models.lseg_net import LSegNet
    cfg = get_config(args.backbone)
    labels = read_labels(os.path.join(ROOT, "lang-seg_amd", "label_files", "ade20k_objectInfo150.txt"))[:args.labels]
    while len(labels) < args.labels:
        labels.append(f"label{len(labels)}")
    K = len(labels)
    net = LSegNet(labels=labels, backbone=args.backbone, features=cfg.features, arch_option=0, block_depth=0, activation="lrelu")
    net.load_state_dict(synthetic_state_dict(cfg, seed=0))
    mod = ModuleSurface(net.cuda().eval(), crop_size=args.crop, base_size=args.base)
    h, w = args.image
    img = synthetic_images(1, h, w, seed=9).cuda()
    geo = [scale_geometry(h, w, s, args.base, args.crop) for s in SCALES]
    crops = [2 * g[4] * g[5] for g in geo]
    windowed = hasattr(__import__("lseg_hip.evaluator", fromlist=["x"]), "window_partition")
    lines = [f"multi-scale evaluator, {args.backbone} crop {args.crop} / base {args.base}, one {h}x{w} image, scales {SCALES} + flip, K = {K}, "
             f"synthetic weights, image_dtype {net.image_dtype}; package from {os.path.relpath(ROOT)} "
             f"({'windows within a scale' if windowed else 'a scale is one stack'})",
             f"grids per scale {[(g[4], g[5]) for g in geo]}: crops with their mirrored twins per scale {crops}, {sum(crops)} in all",
             f"1 warm-up image, then {args.repeats} images; ms per image: median (min .. max); peak = max_memory_allocated of one call above "
             f"the resident tensors", ""]
    results = {}
    for lowres in ([False, True] if args.lowres == "both" else [args.lowres == "1"]):
        tag = f"lowres={lowres}"
        ev = BatchedMultiEval(mod, K, flip=True, scales=SCALES, max_batch=args.max_batch, lowres=lowres)
        if args.max_stack is not None:
            ev.max_stack = args.max_stack
        max_stack = args.max_stack if args.max_stack is not None else (192 if lowres else 48)
        side = args.crop // 2 if lowres else args.crop
        per_crop = K * side * side * 4
        big = max(range(len(geo)), key=lambda i: crops[i])
        maps = (K * h * w + K * geo[big][0] * geo[big][1]) * 4                   # the scores and the largest scale's map
        held = min(max_stack, sum(crops))
        bound = held * per_crop + maps
        inputs = (max(crops) + min(held, args.max_batch, max(crops))) * 3 * args.crop * args.crop * 4
        try:
            with torch.no_grad():
                one_image(ev, img)                                              # engine, text features, allocator pools
                ms = [one_image(ev, img)[0] for _ in range(args.repeats)]
                torch.cuda.synchronize()
                torch.cuda.reset_peak_memory_stats()
                base = torch.cuda.memory_allocated()
                _, out = one_image(ev, img)
                peak = torch.cuda.max_memory_allocated() - base
                results[tag] = out.double().sum().item()
                del out
            lines.append(f"{tag:13s} max_stack {max_stack:4d}  {statistics.median(ms):9.1f} ms ({min(ms):.1f} .. {max(ms):.1f})   peak {peak / 1e6:9.1f} MB   "
                         f"{held} crops x {per_crop / 1e6:.1f} MB + scores and largest map {maps / 1e6:.1f} MB = {bound / 1e6:.1f} MB: "
                         f"{'within' if peak <= bound else 'ABOVE'}; the input crops of the largest scale and one stack's copy of them, "
                         f"not in that bound: {inputs / 1e6:.1f} MB (sum of scores {results[tag]:.6e})")
        except (RuntimeError, torch.cuda.OutOfMemoryError) as e:
            lines.append(f"{tag:13s} max_stack {max_stack:4d}  failed: {type(e).__name__}: {str(e).splitlines()[0][:200]}")
        torch.cuda.empty_cache()
    text = "\n".join(lines)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
