#!/usr/bin/env python
"""Time the ZERO-SHOT training step (LSegNetZS: per-image label pairs, G = 2) next to the LSegNet step with K = 150 shared labels, same
backbone, crop and per-GPU batch, in one process (tools; bench.py is not involved).  Each step: train-mode forward (no full-resolution
logits) + fused cross-entropy + backward + fused SGD, as LSegmentationModule(ZS).training_step -> loss.backward() -> optimizer.step()
drive it.  The engines run one after the other (the first is closed before the second is built).  Prints one JSON line.

    python tools/zs_train_bench.py [--batch 8] [--size 480] [--steps 5] [--warmup 2]

Two further legs, each a same-process A/B in alternating rounds (medians over all timed steps, device events):

    --adam             the fused Adam step (lseg_adam_step) against torch.optim.Adam's step on the same master and gradient tensors
                       followed by the re-pack the engine then needs (lseg_finalize_params) -- what a torch optimizer costs the path
    --freeze-encoder   the whole clip_fixed step with a frozen encoder (truncated backward + fused SGD) against the default clip_fixed
                       step (full backward + torch.optim.SGD on the reference's six groups + re-pack), with the device memory each
                       engine holds after its first step (hipMemGetInfo deltas: the engines allocate outside torch's allocator)
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "lang-seg_amd"))
sys.path.insert(0, ROOT)
import torch                                                                      # noqa: E402
from lseg_hip.config import get_config                                            # noqa: E402
from lseg_hip.engine import HipEngine                                             # noqa: E402
from lseg_hip.synth import synthetic_state_dict, synthetic_tokens, synthetic_images, read_labels   # noqa: E402


def run(cfg, sd, x, tok, target, group, ignore, steps, warmup):
    B, _, H, W = x.shape
    eng = HipEngine(cfg, H, W, max_batch=B, max_labels=tok.shape[0])
    eng.load_state_dict(sd)
    eng.set_tokens(tok, labels_per_image=group)
    eng.enable_training(sd)
    ms = []
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
    eng.close()
    torch.cuda.synchronize()
    med = lambda i: sorted(m[i] for m in ms)[len(ms) // 2]
    return {"step_ms": round(med(0), 2), "forward_ms": round(med(1), 2), "backward_ms": round(med(2), 2), "sgd_ms": round(med(3), 2),
            "step_ms_all": [round(m[0], 2) for m in ms], "loss": float(loss)}


def _used():
    free, total = torch.cuda.mem_get_info()
    return total - free


def _timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1)


def _median(v):
    return round(sorted(v)[len(v) // 2], 3)


def _repack(eng):
    st = torch.cuda.current_stream().cuda_stream
    rc = eng.lib.lseg_finalize_params(eng._h, st)
    assert rc == 0, rc


def _groups(eng, layout):
    """torch parameter groups over the engine's bound masters with the engine's gradients behind .grad"""
    ps = {k: torch.nn.Parameter(eng.bound[k], requires_grad=True) for k in eng.grads}
    for k, p in ps.items():
        assert p.data_ptr() == eng.bound[k].data_ptr()
        p.grad = eng.grads[k]
    if layout == "two":
        return [{"params": [p for k, p in ps.items() if k.startswith("pretrained.")], "lr": 1e-4},
                {"params": [p for k, p in ps.items() if k.startswith("scratch.")], "lr": 1e-3}]
    g = [{"params": [p for k, p in ps.items() if k.startswith("pretrained.model.")], "lr": 0}]          # clip_fixed
    g += [{"params": [p for k, p in ps.items() if k.startswith(f"pretrained.act_postprocess{i}.")], "lr": 1e-4} for i in (1, 2, 3, 4)]
    return g + [{"params": [p for k, p in ps.items() if k.startswith("scratch.")], "lr": 1e-3}]


def _build(cfg, sd, x, tok, freeze):
    B, _, H, W = x.shape
    eng = HipEngine(cfg, H, W, max_batch=B, max_labels=tok.shape[0])
    eng.load_state_dict(sd)
    eng.set_tokens(tok, labels_per_image=2)
    eng.enable_training(sd, freeze_encoder=freeze)
    return eng


def adam_leg(cfg, sd, x, tok, target, steps, warmup, rounds):
    eng = _build(cfg, sd, x, tok, False)
    eng.forward(x, want_logits=False)
    eng.backward(target=target, ignore_index=-100)
    torch.cuda.synchronize()
    opt = torch.optim.Adam(_groups(eng, "two"), lr=1e-4, betas=(0.9, 0.999), weight_decay=1e-4)
    n = sum(v.numel() for v in eng.grads.values())
    t = [0]

    def fused():
        t[0] += 1
        eng.adam_step(1e-4, 1e-3, t[0], weight_decay=1e-4)

    def torch_step():
        opt.step()

    def torch_and_repack():
        opt.step()
        _repack(eng)

    res = {"fused": [], "torch_step": [], "torch_step_repack": []}
    for r in range(rounds):
        for name, fn in (("fused", fused), ("torch_step_repack", torch_and_repack), ("torch_step", torch_step)):
            for s in range(warmup + steps):
                ms = _timed(fn)
                if s >= warmup:
                    res[name].append(ms)
        _repack(eng)                                       # (the bare torch steps left the packs behind)
    eng.close()
    fused_ms = _median(res["fused"])
    return {"parameters": n, "fused_adam_step_ms": fused_ms, "torch_adam_step_ms": _median(res["torch_step"]),
            "torch_adam_step_plus_repack_ms": _median(res["torch_step_repack"]),
            "fused_all_ms": [round(v, 3) for v in res["fused"]], "torch_plus_repack_all_ms": [round(v, 3) for v in res["torch_step_repack"]],
            # 16 B read (w, g, m, v) + 12 B written (w, m, v) per parameter, + 2 B for the 16-bit copy where there is one
            "fused_GBps_at_30B_per_parameter": round(30.0 * n / (fused_ms * 1e-3) / 1e9, 1)}


def frozen_leg(cfg, sd, x, tok, target, steps, warmup, rounds):
    base = _used()
    fz = _build(cfg, {k: v.clone() for k, v in sd.items()}, x, tok, True)

    def frozen_step():
        fz.forward(x, want_logits=False)
        fz.backward(target=target, ignore_index=-100)
        fz.sgd_step(1e-4, 1e-3, 0.9, 1e-4)

    _timed(frozen_step)
    mem_fz = _used() - base
    un = _build(cfg, {k: v.clone() for k, v in sd.items()}, x, tok, False)
    un.forward(x, want_logits=False)
    un.backward(target=target, ignore_index=-100)
    opt = torch.optim.SGD(_groups(un, "six"), lr=1e-4, momentum=0.9, weight_decay=1e-4)

    def default_step():
        un.forward(x, want_logits=False)
        un.backward(target=target, ignore_index=-100)
        opt.step()
        _repack(un)

    _timed(default_step)
    mem_un = _used() - base - mem_fz
    res = {"frozen": [], "default": []}
    for r in range(rounds):
        for name, fn in (("frozen", frozen_step), ("default", default_step)):
            for s in range(warmup + steps):
                ms = _timed(fn)
                if s >= warmup:
                    res[name].append(ms)
    fz.close(); un.close()
    return {"frozen_step_ms": _median(res["frozen"]), "default_clip_fixed_step_ms": _median(res["default"]),
            "frozen_over_default": round(_median(res["frozen"]) / _median(res["default"]), 4),
            "frozen_all_ms": [round(v, 2) for v in res["frozen"]], "default_all_ms": [round(v, 2) for v in res["default"]],
            "device_memory_frozen_GB": round(mem_fz / 2 ** 30, 2), "device_memory_default_GB": round(mem_un / 2 ** 30, 2)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--adam", action="store_true", help="time the fused Adam step against torch.optim.Adam + re-pack")
    ap.add_argument("--freeze-encoder", action="store_true", help="time the frozen-encoder clip_fixed step against the default one")
    ap.add_argument("--rounds", type=int, default=3, help="alternating A/B rounds of the --adam / --freeze-encoder legs")
    ap.add_argument("--backbone", default="clip_vitl16_384")
    ap.add_argument("--size", type=int, default=480)
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--labels", type=int, default=150)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    a = ap.parse_args()
    cfg = get_config(a.backbone)
    sd = {k: v.cuda() for k, v in synthetic_state_dict(cfg, seed=0).items()}
    B, S = a.batch, a.size
    x = synthetic_images(B, S, S, seed=0).cuda()
    g = torch.Generator().manual_seed(1)
    # zero-shot: ['others', class] per image, 0/1 masks, torch's default ignore_index (LSegmentationModuleZS.criterion)
    fss = read_labels(os.path.join(ROOT, "lang-seg_amd", "label_files", "fewshot_fss.txt"), skip_header=False)
    ids = [(7 * i + 3) % len(fss) for i in range(B)]
    tok_zs = torch.cat([synthetic_tokens(["others", fss[c]], cfg.text.vocab, cfg.text.ctx) for c in ids], 0)
    t_zs = torch.randint(0, 2, (B, S, S), generator=g).cuda()
    # LSegNet: K shared ADE20K labels, 20 % ignored pixels (lsegmentation_module.py, ignore_index -1)
    labels = read_labels(os.path.join(ROOT, "lang-seg_amd", "label_files", "ade20k_objectInfo150.txt"))[: a.labels]
    tok = synthetic_tokens(labels, cfg.text.vocab, cfg.text.ctx)
    t = torch.randint(0, len(labels), (B, S, S), generator=g)
    t[torch.rand(t.shape, generator=g) < 0.2] = -1
    t = t.cuda()
    t0 = time.perf_counter()
    if a.adam or a.freeze_encoder:
        out = {"tool": "zs_train_bench", "backbone": a.backbone, "size": S, "batch": B, "steps": a.steps, "warmup": a.warmup, "rounds": a.rounds}
        if a.adam:
            out["adam"] = adam_leg(cfg, sd, x, tok_zs, t_zs, a.steps, a.warmup, a.rounds)
        if a.freeze_encoder:
            out["freeze_encoder"] = frozen_leg(cfg, sd, x, tok_zs, t_zs, a.steps, a.warmup, a.rounds)
        out["wall_s"] = round(time.perf_counter() - t0, 1)
        out["device"] = torch.cuda.get_device_name(0)
        print(json.dumps(out))
        return
    zs = run(cfg, sd, x, tok_zs, t_zs, 2, -100, a.steps, a.warmup)
    shared = run(cfg, sd, x, tok, t, 0, -1, a.steps, a.warmup)
    out = {"tool": "zs_train_bench", "backbone": a.backbone, "size": S, "batch": B, "steps": a.steps, "warmup": a.warmup,
           "zero_shot_G2": zs, f"lsegnet_K{len(labels)}": shared,
           "zs_over_shared": round(zs["step_ms"] / shared["step_ms"], 4), "wall_s": round(time.perf_counter() - t0, 1),
           "device": torch.cuda.get_device_name(0)}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
