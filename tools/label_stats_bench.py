"""Segmentation metrics without the score planes, timed and weighed (csrc/label_stats.hip):
  1. LSegNet.forward_metrics() beside forward_metrics(panel=64): ViT-L/16, 480 x 480, B = 8, K = 150 and K = 1000, synthetic weights --
     ms per call, torch.cuda.max_memory_allocated of one call above the resident tensors, and the DEVICE memory the route takes as
     torch.cuda.mem_get_info sees it (the engine allocates its workspace outside torch's allocator): free memory before the network
     exists minus free memory after two calls, torch's pool left at its high-water mark -- weights, engine and pool together, each route
     measured alone in the process; the engine's max_labels is printed beside it
  2. lseg_op_label_stats on B = 36 maps of 480 x 480: K = 150 (LDS histograms) and K = 20000 (global atomics) -- achieved bytes / s over
     the 10 bytes a pixel carries, against the chip's measured stream rate (6.29 TB/s, float4 copy), beside torch.bincount-based counting
     of the same maps
The paths alternate in one process, `--repeats` times; medians and ranges.  Appends its sections to --out (the file also holds the NLL
bound ratios tests/test_gpu_label_stats.py writes).

    python tools/label_stats_bench.py [--out profiles/label_stats.txt]
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
from lseg_hip.metrics import label_stats                 # noqa: E402
from lseg_hip.synth import synthetic_state_dict, synthetic_images   # noqa: E402

STREAM_TBS = 6.29                                        # HBM3E as measured on the MI355X with a float4 copy


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


def race(paths, repeats):
    for fn in paths.values():
        fn()
    t = {name: [] for name in paths}
    for _ in range(repeats):
        for name, fn in paths.items():
            t[name].append(timed(fn))
    return t


def bincount_counts(lab, tgt, K):
    """the same counters with torch.bincount (shared label set, ignore_index -1)"""
    l, t = lab.reshape(-1).long(), tgt.reshape(-1)
    on = t >= 0
    tin = on & (t < K)
    pred = torch.bincount(l[on], minlength=K)
    gt = torch.bincount(t[tin], minlength=K)
    hit = tin & (l == t)
    inter = torch.bincount(l[hit], minlength=K)
    return torch.cat([torch.stack([hit.sum(), on.sum()]), inter, pred, gt])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--backbone", default="clip_vitl16_384")
    ap.add_argument("--size", type=int, default=480)
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--labels", type=int, nargs="+", default=[150, 1000])
    ap.add_argument("--panel", type=int, default=64)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--skip-net", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    warnings.simplefilter("ignore")
    lines = []
    S = args.size
    if not args.skip_net:
        from modules.models.lseg_net import LSegNet
        cfg = get_config(args.backbone)
        lines += [f"## forward_metrics() vs forward_metrics(panel={args.panel}): {args.backbone}, {S}x{S}, B = {args.batch}, synthetic weights",
                  f"median of {args.repeats} calls per path, alternating in one process; ms per call (min .. max); torch peak = "
                  "torch.cuda.max_memory_allocated of one call above the resident tensors; device = free memory (torch.cuda.mem_get_info) "
                  "before the network exists minus after two calls of the route alone: weights + engine + torch's pool"]
        x = synthetic_images(args.batch, S, S, seed=3).cuda()
        for K in args.labels:
            labels = [f"thing number {i}" for i in range(K)]
            target = torch.randint(-1, K, (args.batch, S, S), generator=torch.Generator().manual_seed(K)).cuda()

            def make():
                net = LSegNet(labels=["wall", "sky"], backbone=args.backbone, features=cfg.features, arch_option=0, block_depth=0, activation="lrelu")
                net.load_state_dict(synthetic_state_dict(cfg, seed=0))
                return net.cuda().eval()

            def drop(net):
                for eng in list(net._engines.values()):
                    eng.close()
                net._engines.clear()

            calls = {"forward_metrics()": lambda net: net.forward_metrics(x, target, labels),
                     f"forward_metrics(panel={args.panel})": lambda net: net.forward_metrics(x, target, labels, panel=args.panel)}
            lines.append(f"K = {K}")
            try:
                device_mb, max_labels = {}, {}
                for name, call in calls.items():                                # each route alone: what it takes from the device
                    torch.cuda.synchronize()
                    torch.cuda.empty_cache()
                    free0 = torch.cuda.mem_get_info()[0]
                    net = make()
                    call(net)
                    call(net)
                    torch.cuda.synchronize()
                    device_mb[name] = (free0 - torch.cuda.mem_get_info()[0]) / 1e6
                    max_labels[name] = net._last_engine.max_labels
                    drop(net)
                    del net
                nets = [make() for _ in calls]                                  # one network per route, alternating for the times
                paths = {name: (lambda call=call, net=net: call(net)) for (name, call), net in zip(calls.items(), nets)}
                a, b = (fn() for fn in paths.values())
                same = a["correct"] == b["correct"] and torch.equal(a["area_inter"], b["area_inter"]) and torch.equal(a["area_union"], b["area_union"])
                # (K <= 157 at out_c 512: forward_lowres takes the fused correlation kernel, the held features the generic one -- the planes
                # differ in their last bits, as include/lseg_hip.h says of lseg_score_features, and a near-tie may fall the other way)
                lines.append(f"  counts equal: {same} (correct {a['correct']} vs {b['correct']}); nll_sum {a['nll_sum']:.6f} vs {b['nll_sum']:.6f} "
                             f"over {a['nll_count']} pixels")
                t = race(paths, args.repeats)
                for name, fn in paths.items():
                    torch.cuda.empty_cache()
                    lines.append(f"  {name:30s} {statistics.median(t[name]):9.2f} ms ({min(t[name]):.2f} .. {max(t[name]):.2f})   torch peak "
                                 f"{peak_of(fn) / 1e6:8.1f} MB   device {device_mb[name]:8.1f} MB (engine max_labels {max_labels[name]})")
                for net in nets:
                    drop(net)
            except (RuntimeError, torch.cuda.OutOfMemoryError) as e:
                lines.append(f"  failed: {type(e).__name__}: {str(e).splitlines()[0][:200]}")
            nets = None
            del nets
            torch.cuda.empty_cache()
        lines.append("")
    B = 36
    lines += [f"## lseg_op_label_stats: B = {B} maps of {S}x{S} (int16 labels + int64 targets = 10 bytes per pixel), stream rate {STREAM_TBS} TB/s",
              f"median of {args.repeats} x 20 back-to-back calls (no host synchronisation inside) beside torch.bincount-based counting of the same maps"]
    for K in (150, 20000):
        g = torch.Generator().manual_seed(K)
        # piecewise-constant maps like masks: 8 x 8 blocks of one label
        blocks = torch.randint(0, K, (B, S // 8, S // 8), generator=g)
        lab = blocks.repeat_interleave(8, 1).repeat_interleave(8, 2).to(torch.int16).cuda()
        tgt = torch.where(torch.rand((B, S, S), generator=g) < 0.8, lab.cpu().long(), torch.randint(-1, K, (B, S, S), generator=g)).cuda()
        counts, flags = label_stats(lab, tgt, K)
        same = torch.equal(counts, bincount_counts(lab, tgt, K))
        # the bare entry with its arguments made once: the wrapper's tensor bookkeeping is not the kernel's time
        import ctypes as C
        from lseg_hip import _lib
        lib = _lib.load()
        raw = (C.c_void_p(lab.data_ptr()), C.c_void_p(tgt.data_ptr()), B, S, S, K, -1, None, None, 0, C.c_void_p(counts.data_ptr()),
               C.c_void_p(flags.data_ptr()), 1, C.c_void_p(torch.cuda.current_stream().cuda_stream))
        paths = {"label_stats": lambda: [lib.lseg_op_label_stats(*raw) for _ in range(20)],
                 "torch.bincount": lambda: [bincount_counts(lab, tgt, K) for _ in range(20)]}
        t = race(paths, args.repeats)
        lines.append(f"K = {K} ({'LDS histograms' if K <= 4096 else 'global atomics'}): equal to the bincount counts: {same}")
        for name in paths:
            ms = statistics.median(t[name]) / 20
            gbs = B * S * S * 10 / (ms * 1e-3) / 1e9
            lines.append(f"  {name:16s} {ms * 1e3:9.1f} us per call ({min(t[name]) / 20 * 1e3:.1f} .. {max(t[name]) / 20 * 1e3:.1f})   "
                         f"{gbs:8.1f} GB/s = {gbs / (STREAM_TBS * 1e3) * 100:5.1f} % of the stream rate")
    lines.append("")
    text = "\n".join(lines)
    print(text)
    if args.out:
        with open(args.out, "a") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
