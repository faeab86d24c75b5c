"""The multi-scale evaluator on the low-resolution logits, timed against the default path: BatchedMultiEval(lowres=True) -- forwards that
stop before output_conv (lseg_forward_lowres) + lseg_op_eval_accumulate_lowres -- beside BatchedMultiEval() on the workload of bench.py's
`eval_multiscale` leg: ViT-L/16, crop 480 / base 520, one 512 x 683 image, 6 scales + flip, K = 150, synthetic weights.  Both paths run
in ONE process, alternating, `--repeats` times `--iters` images each; the table gives the median over the repeats, their spread
(min .. max) and torch.cuda.max_memory_allocated of one image on each path (the engine's own workspace is allocated outside torch's
allocator and is the same for both).  Also one K = 1000 evaluate_random point per path (or the out-of-memory message of a path that
cannot run it), and the two accumulate kernels alone on the largest scale.

    python tools/eval_lowres_bench.py [--out profiles/eval_lowres.txt]
"""
import argparse
import ctypes as C
import os
import statistics
import sys
import time
import warnings

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "lang-seg_amd")]
os.environ.setdefault("LSEG_SYNTHETIC_TOKENS", "1")

import torch                                             # noqa: E402

from lseg_hip import _lib                                # noqa: E402
from lseg_hip.config import get_config                   # noqa: E402
from lseg_hip.evaluator import BatchedMultiEval, ModuleSurface, scale_geometry   # noqa: E402
from lseg_hip.synth import synthetic_state_dict, synthetic_images, read_labels   # noqa: E402

SCALES = (0.5, 0.75, 1.0, 1.25, 1.5, 1.75)


def timed(fn, iters):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(iters):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / iters * 1e3


def peak_of(fn):
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    fn()
    torch.cuda.synchronize()
    return torch.cuda.max_memory_allocated() - base


def kernels_alone(K, crop, h, w, base, iters=5):
    """The two accumulate kernels on the largest scale's stack (random logits): ms, and GB/s on the bytes each must move."""
    lib = _lib.load()
    height, width, ph, pw, hg, wg, stride = scale_geometry(h, w, SCALES[-1], base, crop)
    n = hg * wg
    g = torch.Generator().manual_seed(0)
    low = torch.randn((2 * n, K, crop // 2, crop // 2), generator=g).cuda()
    full = torch.empty((2 * n, K, crop, crop), device="cuda")
    P = lambda t: C.c_void_p(t.data_ptr())                                       # noqa: E731
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    _lib.check(lib.lseg_op_upsample2x_planes(P(low), P(full), 2 * n * K, crop // 2, crop // 2, st))
    out = torch.empty((K, height, width), device="cuda")
    res = {}
    for tag, fn, src in (("full", lib.lseg_op_eval_accumulate, full), ("lowres", lib.lseg_op_eval_accumulate_lowres, low)):
        run = lambda: _lib.check(fn(P(src), P(out), K, height, width, ph, pw, crop, stride, hg, wg, 1, st))    # noqa: E731
        run()
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
        ms = []
        for _ in range(5):
            ev[0].record()
            for _ in range(iters):
                run()
            ev[1].record()
            torch.cuda.synchronize()
            ms.append(ev[0].elapsed_time(ev[1]) / iters)
        nbytes = src.numel() * 4 + out.numel() * 4
        res[tag] = (statistics.median(ms), min(ms), max(ms), nbytes)
    del low, full, out
    torch.cuda.empty_cache()
    return (height, width, n), res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--backbone", default="clip_vitl16_384")
    ap.add_argument("--crop", type=int, default=480)
    ap.add_argument("--base", type=int, default=520)
    ap.add_argument("--image", type=int, nargs=2, default=[512, 683])
    ap.add_argument("--labels", type=int, default=150)
    ap.add_argument("--big-labels", type=int, default=1000)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--iters", type=int, default=2)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    warnings.simplefilter("ignore")
    from modules.models.lseg_net import LSegNet
    cfg = get_config(args.backbone)
    labels = read_labels(os.path.join(ROOT, "lang-seg_amd", "label_files", "ade20k_objectInfo150.txt"))[:args.labels]
    while len(labels) < args.labels:
        labels.append(f"label{len(labels)}")
    net = LSegNet(labels=labels, backbone=args.backbone, features=cfg.features, arch_option=0, block_depth=0, activation="lrelu")
    net.load_state_dict(synthetic_state_dict(cfg, seed=0))
    mod = ModuleSurface(net.cuda().eval(), crop_size=args.crop, base_size=args.base)
    h, w = args.image
    img = synthetic_images(1, h, w, seed=9).cuda()
    crops = [scale_geometry(h, w, s, args.base, args.crop)[4] * scale_geometry(h, w, s, args.base, args.crop)[5] for s in SCALES]
    live = 2 * sum(crops)
    K = len(labels)
    evs = {"lowres=False": BatchedMultiEval(mod, K, flip=True, scales=SCALES), "lowres=True": BatchedMultiEval(mod, K, flip=True, scales=SCALES, lowres=True)}
    lines = [f"multi-scale evaluator, {args.backbone} crop {args.crop} / base {args.base}, one {h}x{w} image, scales {SCALES} + flip, K = {K}, "
             f"synthetic weights, image_dtype {net.image_dtype}",
             f"crops per scale {crops}: {live} crops with their mirrored twins, one stack (max_stack default) on both paths",
             f"median of {args.repeats} repeats x {args.iters} images, the two paths alternating in one process; ms per image (min .. max)", ""]
    t = {k: [] for k in evs}
    peak = {}
    with torch.no_grad():
        got = {k: ev(img) for k, ev in evs.items()}                    # engines, text features, allocator pools
        same = torch.equal(got["lowres=False"], got["lowres=True"])
        del got
        for _ in range(args.repeats):
            for k, ev in evs.items():
                t[k].append(timed(lambda: ev(img), args.iters))
        for k, ev in evs.items():
            peak[k] = peak_of(lambda: ev(img))
    for k in evs:
        med = statistics.median(t[k])
        lines.append(f"{k:13s} {med:9.2f} ms ({min(t[k]):.2f} .. {max(t[k]):.2f})   {1e3 / med:6.2f} images/s   "
                     f"max_memory_allocated above the resident tensors {peak[k] / 1e6:9.1f} MB")
    mf, ml = statistics.median(t["lowres=False"]), statistics.median(t["lowres=True"])
    spread = max(t["lowres=False"]) - min(t["lowres=False"])
    lines.append(f"lowres=True - lowres=False = {ml - mf:+.2f} ms per image (spread of lowres=False: {spread:.2f} ms); "
                 f"lowres=False / lowres=True = {mf / ml:.3f}")
    lines.append(f"scores bit-identical between the two paths (default split-K schedule, same batches): {same}")
    computed = 0.75 * live * K * args.crop * args.crop * 4
    lines.append(f"peak memory: measured difference {(peak['lowres=False'] - peak['lowres=True']) / 1e6:.1f} MB; computed 3/4 x {live} crops x "
                 f"{K} x {args.crop}^2 x 4 B = {computed / 1e6:.1f} MB per copy of the logits alive (the stack is alive twice while the chunks of "
                 f"max_batch are concatenated: up to {2 * computed / 1e6:.1f} MB)")
    lines.append("")
    (height, width, n), kr = kernels_alone(K, args.crop, h, w, args.base)
    lines.append(f"accumulate kernels alone, scale {SCALES[-1]} ({n} boxes + twins -> [{K}, {height}, {width}]), random logits:")
    for tag, name in (("full", "eval_accumulate_kernel"), ("lowres", "eval_accumulate_lowres_kernel")):
        med, lo, hi, nbytes = kr[tag]
        lines.append(f"  {name:30s} {med:7.3f} ms ({lo:.3f} .. {hi:.3f})   {nbytes / 1e6:8.1f} MB to move -> {nbytes / (med * 1e-3) / 1e9:6.0f} GB/s")
    lines.append("")
    # ---- K = 1000 through evaluate_random ------------------------------------------------------------------------------------
    big = [f"thing number {i}" for i in range(args.big_labels)]
    lines.append(f"K = {args.big_labels} (evaluate_random, label set encoded once), same image, 1 image after 1 warm-up; "
                 f"full-resolution logits of the stack: {live * args.big_labels * args.crop * args.crop * 4 / 1e9:.1f} GB")
    for k, ev in evs.items():
        try:
            with torch.no_grad():
                ev(img, big)
                ms = timed(lambda: ev(img, big), 1)
                pk = peak_of(lambda: ev(img, big))
            lines.append(f"{k:13s} {ms:9.2f} ms   max_memory_allocated above the resident tensors {pk / 1e6:9.1f} MB")
        except (RuntimeError, torch.cuda.OutOfMemoryError) as e:
            lines.append(f"{k:13s} failed: {type(e).__name__}: {str(e).splitlines()[0][:200]}")
        torch.cuda.empty_cache()
    text = "\n".join(lines)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
