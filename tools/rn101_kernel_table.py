"""Per-family kernel table of the zero-shot ResNet-101 network from a `rocprofv3 --kernel-trace` database of tools/rn101_zs_bench.py
(`--only rn101`): every forward's dispatches on the main stream are walked in plan order (stem, max-pool, then per bottleneck conv1, conv2,
[downsample], conv3 -- each a GEMM launch, followed by its split-K reduction when it has one), the rest of the forward is the shared neck /
head, the side stream is the text tower.  FLOP / byte shares against the MI355X's dense fp16 MFMA peak and HBM bandwidth.

    python tools/rn101_kernel_table.py <rocpd .db> --batch 4
"""
import argparse
import collections
import os
import sqlite3
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from rn101_zs_bench import rn101_model  # noqa: E402

PEAK_TFLOPS = 2500.0      # MI355X dense fp16 / bf16 MFMA (MI355X_MICROARCH.md)
PEAK_TBS = 8.0            # HBM3E


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("db")
    ap.add_argument("--batch", type=int, default=4)
    ap.add_argument("--last", type=int, default=5, help="forwards averaged (the last N)")
    a = ap.parse_args()
    c = sqlite3.connect(a.db)
    rows = c.execute("select name, stream_id, start, end from kernels order by start").fetchall()
    stems = [i for i, r in enumerate(rows) if "::rn_stem_kernel(" in r[0]]
    main_stream = rows[stems[0]][1]
    fwd = []
    for s_i, s in enumerate(stems):
        end = stems[s_i + 1] if s_i + 1 < len(stems) else len(rows)
        seq = [r for r in rows[s:end] if r[1] == main_stream and "fillBuffer" not in r[0]]
        fam = collections.defaultdict(float)
        t0 = seq[0][2]
        fam["stem"] += (seq[0][3] - seq[0][2]) / 1e3
        fam["maxpool"] += (seq[1][3] - seq[1][2]) / 1e3
        k = 2
        for l, n in enumerate((3, 4, 23, 3)):
            for j in range(n):
                for f in ("conv1x1", "conv3x3") + (("downsample",) if j == 0 else ()) + ("conv1x1",):
                    assert "gemm" in seq[k][0], seq[k][0]
                    fam[f] += (seq[k][3] - seq[k][2]) / 1e3
                    k += 1
                    if k < len(seq) and "conv_reduce_pad" in seq[k][0]:
                        fam[f + " split-K reduce"] += (seq[k][3] - seq[k][2]) / 1e3
                        k += 1
        tower_end = seq[k - 1][3]
        for r in seq[k:]:
            fam["neck + head (shared with ViT)"] += (r[3] - r[2]) / 1e3
        fam["forward wall (main stream)"] = (seq[-1][3] - t0) / 1e3
        fam["tower wall"] = (tower_end - t0) / 1e3
        fwd.append(fam)
    fwd = fwd[-a.last:]
    keys = list(fwd[-1].keys())
    model = rn101_model(a.batch)
    print(f"ResNet-101 zero-shot forward, 480x480, B = {a.batch}, fp16; mean of {len(fwd)} forwards (rocprofv3 --kernel-trace)")
    print(f"{'family':34s} {'us':>9s} {'GFLOP':>8s} {'MB':>8s} {'MFMA %':>7s} {'HBM %':>6s}")
    for key in keys:
        us = sum(f[key] for f in fwd) / len(fwd)
        m = model.get(key)
        if m:
            fl, by = m
            print(f"{key:34s} {us:9.1f} {fl / 1e9:8.2f} {by / 1e6:8.1f} {100 * fl / (us * 1e-6) / (PEAK_TFLOPS * 1e12):7.1f} "
                  f"{100 * by / (us * 1e-6) / (PEAK_TBS * 1e12):6.1f}")
        else:
            print(f"{key:34s} {us:9.1f}")


if __name__ == "__main__":
    main()
