"""The cross-entropy on the streamed label route, timed and weighed (csrc/corr_argmax.hip LOSS; lseg_forward_labels_loss):
  1. LSegNet.forward_metrics(streamed=True) beside forward_metrics() at K = 150, and beside forward_metrics() and
     forward_metrics(panel=64) at K = 1000: ViT-L/16, 480 x 480, B = 8, synthetic weights -- ms per call, torch.cuda.max_memory_allocated
     of one call above the resident tensors, and the DEVICE memory the route takes as torch.cuda.mem_get_info sees it (weights + engine +
     torch's pool, each route alone in a fresh network), measured as tools/label_stats_bench.py measures them
  2. per-image label lists of 2 .. 150 labels at B = 8: forward_metrics(streamed=True) in eval mode beside a train-mode ragged forward +
     loss value (LSegNet.forward_loss without the backward: the only route to the ragged loss value before this one)
The paths alternate in one process, `--repeats` times; medians and ranges.

    python tools/streamed_loss_bench.py [--out profiles/streamed_loss.txt]
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
from lseg_hip.synth import synthetic_state_dict, synthetic_images   # noqa: E402


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


def drop(net):
    for eng in list(net._engines.values()):
        eng.close()
    net._engines.clear()


def compare(lines, make, calls, repeats, describe):
    """each route alone in a fresh network (device memory), then one network per route alternating (times, torch peak)"""
    try:
        device_mb = {}
        for name, call in calls.items():
            torch.cuda.synchronize()
            torch.cuda.empty_cache()
            free0 = torch.cuda.mem_get_info()[0]
            net = make()
            call(net)
            call(net)
            torch.cuda.synchronize()
            device_mb[name] = (free0 - torch.cuda.mem_get_info()[0]) / 1e6
            drop(net)
            del net
        nets = [make() for _ in calls]
        paths = {name: (lambda call=call, net=net: call(net)) for (name, call), net in zip(calls.items(), nets)}
        lines.append("  " + describe([fn() for fn in paths.values()]))
        t = race(paths, repeats)
        for name, fn in paths.items():
            torch.cuda.empty_cache()
            lines.append(f"  {name:34s} {statistics.median(t[name]):9.2f} ms ({min(t[name]):.2f} .. {max(t[name]):.2f})   torch peak "
                         f"{peak_of(fn) / 1e6:8.1f} MB   device {device_mb[name]:8.1f} MB")
        for net in nets:
            drop(net)
    except (RuntimeError, torch.cuda.OutOfMemoryError) as e:
        lines.append(f"  failed: {type(e).__name__}: {str(e).splitlines()[0][:200]}")
    torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--backbone", default="clip_vitl16_384")
    ap.add_argument("--size", type=int, default=480)
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--panel", type=int, default=64)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    warnings.simplefilter("ignore")
    from modules.models.lseg_net import LSegNet
    cfg = get_config(args.backbone)
    S, B = args.size, args.batch
    x = synthetic_images(B, S, S, seed=3).cuda()

    def make():
        net = LSegNet(labels=["wall", "sky"], backbone=args.backbone, features=cfg.features, arch_option=0, block_depth=0, activation="lrelu")
        net.load_state_dict(synthetic_state_dict(cfg, seed=0))
        return net.cuda().eval()

    lines = [f"## forward_metrics(streamed=True) beside the routes that hold logits: {args.backbone}, {S}x{S}, B = {B}, synthetic weights",
             f"median of {args.repeats} calls per path, alternating in one process; ms per call (min .. max); torch peak = "
             "torch.cuda.max_memory_allocated of one call above the resident tensors; device = free memory (torch.cuda.mem_get_info) "
             "before the network exists minus after two calls of the route alone: weights + engine + torch's pool"]
    for K in (150, 1000):
        labels = [f"thing number {i}" for i in range(K)]
        target = torch.randint(-1, K, (B, S, S), generator=torch.Generator().manual_seed(K)).cuda()
        calls = {"forward_metrics()": lambda net: net.forward_metrics(x, target, labels)}
        if K > 150:
            calls[f"forward_metrics(panel={args.panel})"] = lambda net: net.forward_metrics(x, target, labels, panel=args.panel)
        calls["forward_metrics(streamed=True)"] = lambda net: net.forward_metrics(x, target, labels, streamed=True)
        lines.append(f"K = {K}")

        def describe(rs):
            a, s = rs[0], rs[-1]
            same = a["correct"] == s["correct"] and torch.equal(a["area_inter"], s["area_inter"]) and torch.equal(a["area_union"], s["area_union"])
            return (f"streamed counts equal forward_metrics(): {same} (correct {s['correct']} vs {a['correct']}); nll_sum {s['nll_sum']:.6f} vs "
                    f"{a['nll_sum']:.6f} over {s['nll_count']} pixels")
        compare(lines, make, calls, args.repeats, describe)
    lines.append("")

    counts = [2 + round(b * 148 / max(B - 1, 1)) for b in range(B)]
    lists = [[f"thing number {i} of image {b}" for i in range(k)] for b, k in enumerate(counts)]
    g = torch.Generator().manual_seed(7)
    target = torch.stack([torch.randint(-1, k, (S, S), generator=g) for k in counts]).cuda()
    lines += [f"## per-image label lists of {counts} labels, B = {B}: the loss value in eval mode (streamed) beside a train-mode forward + loss",
              "(train mode: bf16 operands, saved activations, batch-statistics BatchNorm; the values are not expected to agree)"]

    def train_value(net):
        net.train()
        with torch.enable_grad():
            v = net.forward_loss(x, target, lists, ignore_index=-1).item()
        net.eval()
        return {"loss": v}

    def streamed_value(net):
        r = net.forward_metrics(x, target, lists, ignore_index=-1, streamed=True)
        return {"loss": r["nll_sum"] / max(r["nll_count"], 1)}

    compare(lines, make, {"train forward + forward_loss value": train_value, "forward_metrics(streamed=True)": streamed_value}, args.repeats,
            lambda rs: f"mean loss: train-mode {rs[0]['loss']:.6f}, streamed eval {rs[1]['loss']:.6f}")
    lines.append("")
    text = "\n".join(lines)
    print(text)
    if args.out:
        with open(args.out, "a") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
