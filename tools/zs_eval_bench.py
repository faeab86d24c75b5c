"""Few-shot episode evaluation step, timed: LSeg.evaluate_episode + EpisodeMeter (one inference forward without full-resolution logits,
one statistics launch; csrc/episode.hip) against what a user ran before it existed -- net.forward -> argmax -> cross_entropy -> the
torch area bookkeeping of tests/episode_helpers.py -> index_add_ -- on LSegNetZS ViT-L/16 at 480 x 480, B = 20 (the reference's bsz,
test_lseg_zs.py) and B = 1, synthetic weights.  Both paths are timed in ONE process, interleaved, `--repeats` times `--iters` steps each;
the table gives the median over the repeats and their spread (min .. max).  Also the bare kernel's achieved GB/s on the bytes it must
read: the 2 low-resolution planes (fp32), the target (8 B / pixel) and the ignore mask (1 B / pixel).

    python tools/zs_eval_bench.py [--out profiles/zs_episode_eval.txt]
"""
import argparse
import ctypes as C
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "lang-seg_amd"), os.path.join(ROOT, "tests")]
os.environ.setdefault("LSEG_SYNTHETIC_TOKENS", "1")

import torch                                             # noqa: E402
import torch.nn.functional as F                          # noqa: E402

import episode_helpers as eh                             # noqa: E402
from lseg_hip import _lib                                # noqa: E402
from lseg_hip.episode import EpisodeMeter                # noqa: E402
from lseg_hip.synth import synthetic_state_dict, synthetic_images   # noqa: E402


def timed(fn, iters):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(iters):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / iters * 1e3


def kernel_gbs(B, H, W, iters=50):
    lib = _lib.load()
    g = torch.Generator().manual_seed(1)
    low = torch.randn(B, 2, H // 2, W // 2, generator=g).cuda()
    target = torch.randint(0, 2, (B, H, W), generator=g).cuda()
    ignore = (torch.rand(B, H, W, generator=g) < 0.1).to(torch.uint8).cuda() * (target == 0).to(torch.uint8)
    ws = torch.empty(max(1, lib.lseg_op_episode_stats_ws_bytes(B, H, W) // 8), dtype=torch.float64, device="cuda")
    areas = torch.empty(B, 6, dtype=torch.int64, device="cuda")
    nll = torch.empty(B, 2, dtype=torch.float64, device="cuda")
    flags = torch.empty(2, dtype=torch.int64, device="cuda")
    P = lambda t: C.c_void_p(t.data_ptr())                                       # noqa: E731
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)

    def run():
        _lib.check(lib.lseg_op_episode_stats(P(low), P(target), P(ignore), B, H, W, 1, -100, None, 0, None, None, P(areas), P(nll), P(flags),
                                             P(ws), ws.numel() * 8, st))
    for _ in range(5):
        run()
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    ms = []
    for _ in range(7):
        ev[0].record()
        for _ in range(iters):
            run()
        ev[1].record()
        torch.cuda.synchronize()
        ms.append(ev[0].elapsed_time(ev[1]) / iters)
    nbytes = B * (2 * (H // 2) * (W // 2) * 4 + H * W * 8 + H * W)
    med = statistics.median(ms)
    return med, min(ms), max(ms), nbytes, nbytes / (med * 1e-3) / 1e9


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--backbone", default="clip_vitl16_384")
    ap.add_argument("--size", type=int, default=480)
    ap.add_argument("--batches", type=int, nargs="+", default=[20, 1])
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    from modules.models.lseg_net_zs import LSegNetZS
    nclass = 20
    names = [f"class{i}" for i in range(nclass)]
    net = LSegNetZS(label_list=names, backbone=args.backbone, features=256, aux=False, use_pretrained=False, arch_option=0, block_depth=0,
                    activation="lrelu")
    net.load_state_dict(synthetic_state_dict(net.cfg, seed=0), strict=False)
    net = net.cuda().eval()
    H = W = args.size
    lines = [f"few-shot episode evaluation step, {args.backbone} {H}x{W}, synthetic weights, image_dtype {net.image_dtype}",
             f"median of {args.repeats} repeats x {args.iters} steps, both paths interleaved in one process; ms per step (min .. max)",
             "  new    = LSeg.evaluate_episode(x, class_info, target, ignore, meter)            [forward without logits + lseg_episode_stats]",
             "  logits = net(x, class_info) -> argmax -> F.cross_entropy -> torch areas (tests/episode_helpers.classify) -> index_add_", ""]
    for B in args.batches:
        g = torch.Generator().manual_seed(B)
        x = synthetic_images(B, H, W, seed=B).cuda()
        ids = [(3 * i) % nclass for i in range(B)]
        target = torch.randint(0, 2, (B, H, W), generator=g).cuda()
        ignore = ((torch.rand(B, H, W, generator=g) < 0.1).cuda() & (target == 0)).to(torch.uint8)
        meter = EpisodeMeter(nclass, range(nclass), "cuda")
        ibuf = torch.zeros(2, nclass, device="cuda")
        ubuf = torch.zeros(2, nclass, device="cuda")
        cid = torch.tensor(ids, device="cuda")

        def new():
            meter.loss_buf.clear()
            net.evaluate_episode(x, ids, target, ignore=ignore, meter=meter)

        def old():
            out = net(x, ids)
            loss = F.cross_entropy(out.view(B, 2, -1), target.view(B, -1))
            inter, union = eh.inter_union(eh.classify(out.argmax(1), target, ignore))
            ibuf.index_add_(1, cid, inter.float())
            ubuf.index_add_(1, cid, union.float())
            return loss

        with torch.no_grad():
            for _ in range(2):
                new()
                old()
            tn, to = [], []
            for _ in range(args.repeats):
                tn.append(timed(new, args.iters))
                to.append(timed(old, args.iters))
        mn, mo = statistics.median(tn), statistics.median(to)
        lines.append(f"B = {B:2d}   new    {mn:8.3f} ms ({min(tn):.3f} .. {max(tn):.3f})   {B / mn * 1e3:7.1f} img/s")
        lines.append(f"         logits {mo:8.3f} ms ({min(to):.3f} .. {max(to):.3f})   {B / mo * 1e3:7.1f} img/s   logits / new = {mo / mn:.3f}")
        med, lo, hi, nbytes, gbs = kernel_gbs(B, H, W)
        lines.append(f"         episode_stats_kernel + fold alone (up = 1): {med * 1e3:.1f} us ({lo * 1e3:.1f} .. {hi * 1e3:.1f}), {nbytes / 1e6:.2f} MB to read "
                     f"-> {gbs:.0f} GB/s achieved")
        lines.append("")
    text = "\n".join(lines)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
