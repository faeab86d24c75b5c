"""Images/s of the zero-shot CLIP-ResNet-101 network (LSegRNNetZS's engine, lseg_config.flags bit 5) at 480 x 480 against the ViT-L/16
zero-shot network (LSegNetZS's engine) in the same process at the same batch, plus the FLOP / byte model of the ResNet tower's kernel
families from shapes (the per-kernel times come from a separate `rocprofv3 --kernel-trace --stats` run of `--only rn101`).

    python tools/rn101_zs_bench.py [--batches 1 4 16] [--dtypes fp16 bf16] [--only rn101|vitl16] [--windows 3] [--iters 10]

Every timed window ends in a device synchronisation; the median of the windows is reported.  One JSON line per (network, dtype, B).
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "lang-seg_amd")]

import torch  # noqa: E402

from lseg_hip.config import get_config  # noqa: E402
from lseg_hip.engine import HipEngine  # noqa: E402
from lseg_hip.synth import synthetic_images, synthetic_state_dict, synthetic_tokens  # noqa: E402

H = W = 480
NETS = {"rn101": "clip_resnet101", "vitl16": "clip_vitl16_384"}


def rn101_model(B, H=480, W=480):
    """FLOPs (2 per MAC) and compulsory HBM bytes (16-bit maps written once and read once per consumer) of the tower's families."""
    fam = {k: [0.0, 0.0] for k in ("stem", "maxpool", "conv1x1", "conv3x3", "downsample")}
    h, w = H // 2, W // 2
    fam["stem"][0] += 2.0 * B * h * w * 64 * 147
    fam["stem"][1] += B * 3 * H * W * 4 + B * h * w * 64 * 2
    fam["maxpool"][1] += B * h * w * 64 * 2 + B * (h // 2) * (w // 2) * 64 * 2
    h, w, cin = h // 2, w // 2, 64
    for l, n in enumerate((3, 4, 23, 3)):
        wd = 64 << l
        for j in range(n):
            s = 2 if (j == 0 and l > 0) else 1
            ho, wo = h // s, w // s
            fam["conv1x1"][0] += 2.0 * B * h * w * cin * wd + 2.0 * B * ho * wo * wd * 4 * wd
            fam["conv1x1"][1] += 2 * B * (h * w * (cin + wd) + ho * wo * (wd + 4 * wd * 2))
            fam["conv3x3"][0] += 2.0 * B * ho * wo * 9 * wd * wd
            fam["conv3x3"][1] += 2 * B * (h * w * wd + ho * wo * wd)
            if j == 0:
                fam["downsample"][0] += 2.0 * B * ho * wo * cin * 4 * wd
                fam["downsample"][1] += 2 * B * (h * w * cin + ho * wo * 4 * wd)
            h, w, cin = ho, wo, 4 * wd
    return fam


def make_engine(net, B, dtype):
    cfg = get_config(NETS[net])
    eng = HipEngine(cfg, H, W, max_batch=B, max_labels=2 * B, image_dtype=dtype)
    eng.load_state_dict(synthetic_state_dict(cfg, seed=0))
    labels = []
    for b in range(B):
        labels += ["others", f"class{b}"]
    eng.set_tokens(synthetic_tokens(labels), labels_per_image=2)
    return eng


def bench(eng, x, windows, iters, warmup=3):
    for _ in range(warmup):
        eng.forward(x)
    torch.cuda.synchronize()
    ts = []
    for _ in range(windows):
        t0 = time.perf_counter()
        for _ in range(iters):
            eng.forward(x)
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) / iters)
    ts.sort()
    return ts[len(ts) // 2], ts


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", type=int, nargs="+", default=[1, 4, 16])
    ap.add_argument("--dtypes", nargs="+", default=["fp16", "bf16"])
    ap.add_argument("--only", choices=list(NETS), default=None)
    ap.add_argument("--windows", type=int, default=3)
    ap.add_argument("--iters", type=int, default=10)
    a = ap.parse_args()
    torch.cuda.set_device(0)
    nets = [a.only] if a.only else list(NETS)
    for dtype in a.dtypes:
        for B in a.batches:
            x = synthetic_images(B, H, W, seed=1).cuda()
            res = {}
            for net in nets:
                eng = make_engine(net, B, dtype)
                med, ts = bench(eng, x, a.windows, a.iters)
                res[net] = med
                line = {"net": net, "dtype": dtype, "B": B, "ms": round(med * 1e3, 3), "img_s": round(B / med, 1),
                        "windows_ms": [round(t * 1e3, 3) for t in ts]}
                if net == "rn101":
                    line["tower_gflop"] = round(sum(v[0] for v in rn101_model(B).values()) / 1e9, 1)
                print(json.dumps(line), flush=True)
                eng.close()
                del eng
                torch.cuda.empty_cache()
            if len(res) == 2:
                print(json.dumps({"dtype": dtype, "B": B, "rn101_over_vitl16_time": round(res["rn101"] / res["vitl16"], 3)}), flush=True)
    print(json.dumps({"model_B4": {k: {"gflop": round(v[0] / 1e9, 2), "mb": round(v[1] / 1e6, 1)} for k, v in rn101_model(4).items()}}))


if __name__ == "__main__":
    main()
