#!/usr/bin/env python
"""Time the RAGGED training step (per-image label lists of different lengths, lseg_set_text_groups in train mode) next to the shared-set
step at K = 150, same backbone, crop and batch, in one process (tools; bench.py is not involved).  Each step: train-mode forward (no
full-resolution logits) + fused cross-entropy + backward + fused SGD.  Both engines are alive and take turns in alternating rounds;
the medians run over all timed steps of all rounds.  The ragged step runs on the one-launch correlation kernels (stage two); the same
pair of legs is then measured by a fresh child process under LSEG_CORR_RAGGED_GEMM=1 (the switch is read once per process), where the
ragged correlation runs per image on the generic GEMM (stage one).
Prints one JSON line and, with --out, rewrites the step-time section of the report (everything from the line that starts with
"2. Step times" on; what stands above it -- the kernels' error figures -- is kept).

    python tools/ragged_train_bench.py [--batch 8] [--size 480] [--steps 5] [--warmup 2] [--rounds 3] [--out profiles/ragged_train.txt]
"""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "lang-seg_amd"))
sys.path.insert(0, ROOT)
import torch                                                                      # noqa: E402
from lseg_hip.config import get_config                                            # noqa: E402
from lseg_hip.engine import HipEngine                                             # noqa: E402
from lseg_hip.synth import synthetic_state_dict, synthetic_tokens, synthetic_images, read_labels   # noqa: E402


def build(cfg, sd, x, tok, counts):
    B, _, H, W = x.shape
    sd = {k: v.clone() for k, v in sd.items()}            # each engine steps its own masters
    eng = HipEngine(cfg, H, W, max_batch=B, max_labels=tok.shape[0])
    eng.load_state_dict(sd)
    eng.set_tokens(tok, group_sizes=counts)
    eng.enable_training(sd)
    return eng


def timed_steps(eng, x, target, ignore, steps, warmup, ms):
    for s in range(warmup + steps):
        e0, e1, e2, e3 = (torch.cuda.Event(enable_timing=True) for _ in range(4))
        e0.record()
        eng.forward(x, want_logits=False)
        e1.record()
        loss = eng.backward(target=target, ignore_index=ignore)
        e2.record()
        eng.sgd_step(1e-4, 1e-3, 0.9, 1e-4)
        e3.record()
        torch.cuda.synchronize()
        if s >= warmup:
            ms.append((e0.elapsed_time(e3), e0.elapsed_time(e1), e1.elapsed_time(e2), e2.elapsed_time(e3)))
    return float(loss)


def summary(ms, loss):
    med = lambda i: sorted(m[i] for m in ms)[len(ms) // 2]
    return {"step_ms": round(med(0), 2), "forward_ms": round(med(1), 2), "backward_ms": round(med(2), 2), "sgd_ms": round(med(3), 2),
            "step_ms_all": [round(m[0], 2) for m in ms], "loss": loss}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--backbone", default="clip_vitl16_384")
    ap.add_argument("--size", type=int, default=480)
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--rounds", type=int, default=3, help="alternating rounds of the two engines")
    ap.add_argument("--out", default="")
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    a = ap.parse_args()
    cfg = get_config(a.backbone)
    sd = {k: v.cuda() for k, v in synthetic_state_dict(cfg, seed=0).items()}
    B, S = a.batch, a.size
    x = synthetic_images(B, S, S, seed=0).cuda()
    g = torch.Generator().manual_seed(1)
    labels = read_labels(os.path.join(ROOT, "lang-seg_amd", "label_files", "ade20k_objectInfo150.txt"))[:150]
    # lists of 2 ... 150 labels, spread evenly over the batch, each a prefix of the vocabulary rotated by the image index
    counts = [2 + round((150 - 2) * b / max(B - 1, 1)) for b in range(B)]
    lists = [[labels[(i + 11 * b) % len(labels)] for i in range(k)] for b, k in enumerate(counts)]
    tok_r = synthetic_tokens([w for ls in lists for w in ls], cfg.text.vocab, cfg.text.ctx)
    ign = torch.rand((B, S, S), generator=g) < 0.2
    u = torch.rand((B, S, S), generator=g)
    t_r = torch.stack([(u[b] * counts[b]).long().clamp(max=counts[b] - 1) for b in range(B)])
    t_r[ign] = -1
    tok_s = synthetic_tokens(labels, cfg.text.vocab, cfg.text.ctx)
    t_s = (u * len(labels)).long().clamp(max=len(labels) - 1)
    t_s[ign] = -1
    t0 = time.perf_counter()
    er, es = build(cfg, sd, x, tok_r, counts), build(cfg, sd, x, tok_s, None)
    t_r, t_s = t_r.cuda(), t_s.cuda()
    mr, ms_ = [], []
    for _ in range(a.rounds):
        lr_ = timed_steps(er, x, t_r, -1, a.steps, a.warmup, mr)
        ls_ = timed_steps(es, x, t_s, -1, a.steps, a.warmup, ms_)
    er.close(); es.close()
    torch.cuda.synchronize()
    ragged, shared = summary(mr, lr_), summary(ms_, ls_)
    out = {"tool": "ragged_train_bench", "backbone": a.backbone, "size": S, "batch": B, "steps": a.steps, "warmup": a.warmup, "rounds": a.rounds,
           "counts": counts, "labels_in_all": sum(counts), "ragged_per_image_gemm" if os.environ.get("LSEG_CORR_RAGGED_GEMM") is not None else "ragged_one_launch": ragged, f"shared_K{len(labels)}": shared,
           "ragged_over_shared": round(ragged["step_ms"] / shared["step_ms"], 4), "wall_s": round(time.perf_counter() - t0, 1),
           "device": torch.cuda.get_device_name(0)}
    out["ragged_correlation"] = "per-image GEMM (LSEG_CORR_RAGGED_GEMM)" if os.environ.get("LSEG_CORR_RAGGED_GEMM") is not None else "one launch"
    if a.child:
        print(json.dumps(out))
        return
    env = dict(os.environ, LSEG_CORR_RAGGED_GEMM="1")
    args = [sys.executable, os.path.abspath(__file__), "--child", "--backbone", a.backbone, "--size", str(S), "--batch", str(B), "--steps", str(a.steps),
            "--warmup", str(a.warmup), "--rounds", str(a.rounds)]
    child = json.loads(subprocess.check_output(args, env=env, text=True).strip().splitlines()[-1])
    out["stage_one_process"] = child
    g1 = child["ragged_per_image_gemm"]
    line = json.dumps(out)
    print(line)
    if a.out:
        keep = ""
        if os.path.exists(a.out):
            old = open(a.out).read()
            i = old.find("2. Step times")
            keep = old if i < 0 else old[:i]
        with open(a.out, "w") as f:
            f.write(keep + "2. Step times (tools/ragged_train_bench.py)\n\n")
            f.write(f"ragged training step, {a.backbone} {S}x{S}, B = {B}, lists of {counts} labels ({sum(counts)} in all); medians over "
                    f"{a.rounds} alternating rounds of {a.steps} steps after {a.warmup} warm-up steps each, device events, one process\n"
                    f"  ragged step, one-launch correlation         {ragged['step_ms']:8.2f} ms  (forward {ragged['forward_ms']}, backward "
                    f"{ragged['backward_ms']}, sgd {ragged['sgd_ms']})\n"
                    f"  shared-set step, K = {len(labels)}                  {shared['step_ms']:8.2f} ms  (forward {shared['forward_ms']}, backward "
                    f"{shared['backward_ms']}, sgd {shared['sgd_ms']})\n"
                    f"  ragged / shared                            {out['ragged_over_shared']:8.4f}\n"
                    f"  second process, LSEG_CORR_RAGGED_GEMM=1 (per-image GEMM correlation):\n"
                    f"  ragged step, per-image GEMM correlation     {g1['step_ms']:8.2f} ms  (forward {g1['forward_ms']}, backward {g1['backward_ms']}, "
                    f"sgd {g1['sgd_ms']}); shared-set step there {child['shared_K150']['step_ms']:.2f} ms\n" + line + "\n")


if __name__ == "__main__":
    main()
