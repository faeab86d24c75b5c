"""Bit identity of two builds of liblseg_hip.so: sha256 of every output tensor of a fixed list of small cases that together reach each
GEMM descriptor and stage the forwards, the text tower and the backward share (csrc/engine.h builders, Engine::patch_embed /
reassemble / out_conv / correlate_planes), every output tail of Engine::forward (csrc/forward_route.h) and every mode and stage of the
training step's label head (csrc/train_head.h) with the three encoder tails of the backward.  A host-side restructuring of the schedule
must leave every line unchanged.  (The loss VALUES are double atomic sums, whose last bits may depend on the order the workgroups arrive
in: run the older library twice and leave out the lines that differ between its own runs -- profiles/train_refactor.txt: none did.)

    python tools/ab_bit_identity.py --lib OLD/liblseg_hip.so --out old.txt
    python tools/ab_bit_identity.py --out new.txt          # the in-tree build
    diff old.txt new.txt                                   # must be empty; the last line of each is the case count + overall hash

One fresh interpreter per case (the library is chosen through LSEG_HIP_LIB), each under its own time limit; the run stops at the first
child that does not exit 0 and returns its status.  `--cases a,b` selects, `--list` names them.
"""
import argparse
import hashlib
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "lang-seg_amd")]

LABELS = ["wall", "sky", "tree", "floor", "other", "road", "grass"]


def emit(case, name, t):
    import torch
    t = t.detach().contiguous().cpu()
    raw = t.reshape(-1).view(torch.uint8).numpy().tobytes() if t.numel() else b""
    print(f"{case} {name} {str(t.dtype).replace('torch.', '')}{list(t.shape)} {hashlib.sha256(raw).hexdigest()}", flush=True)


def engine(backbone, S, B, K, dtype, group=0, width=None, **kw):
    from lseg_hip.config import get_config
    from lseg_hip.engine import HipEngine
    from lseg_hip.synth import synthetic_state_dict, synthetic_tokens, synthetic_images
    cfg = get_config(backbone, arch_option=kw.pop("arch_option", 0), block_depth=kw.pop("block_depth", 0))
    sd = {k: v.cuda() for k, v in synthetic_state_dict(cfg, seed=7).items()}
    eng = HipEngine(cfg, S, width or S, max_batch=B, max_labels=K, image_dtype=dtype, deterministic=True, **kw)
    eng.load_state_dict(sd)
    eng.set_tokens(synthetic_tokens([LABELS[i % len(LABELS)] for i in range(K)], cfg.text.vocab, cfg.text.ctx), labels_per_image=group)
    return eng, sd, synthetic_images(B, S, width or S, seed=7).cuda()


def run_eval(case, backbone, S, B, K, dtypes, group=0, debug=False, text_features=False, **kw):
    import torch
    for dt in dtypes:
        eng, _, x = engine(backbone, S, B, K, dt, group, **kw)
        if text_features:                                       # the tower's own features handed back in, scaled: the engine normalises
            eng.set_text_features(eng.encode_text() * 3.0)
        eng.set_debug(debug)
        kout = group if group else K
        emit(case, f"{dt}.logits", eng.forward(x))
        emit(case, f"{dt}.lowres", eng.intermediate("lowres", (B, kout, S // 2, S // 2)))
        emit(case, f"{dt}.masks", eng.forward(x, want_logits=False, want_argmax=True))
        lab, score = eng.forward_labels(x, want_score=True)
        emit(case, f"{dt}.labels", lab)
        emit(case, f"{dt}.score", score)
        if debug and eng.cfg.tower != "resnet101":
            ntok = (S // eng.cfg.patch) ** 2 + 1
            for l in range(4):
                emit(case, f"{dt}.act{l + 1}", eng.intermediate(f"act{l + 1}", (B, ntok, eng.cfg.dim)))
        torch.cuda.synchronize()
        eng.close()


def run_train(case, backbone, S, B, K, group=0, freeze=False, **kw):
    import torch
    eng, sd, x = engine(backbone, S, B, K, "bf16", group, **kw)
    eng.enable_training(sd, freeze_encoder=freeze)
    kout = group if group else K
    target = torch.randint(0, kout, (B, S, kw.get("width") or S), generator=torch.Generator().manual_seed(11)).cuda()
    emit(case, "logits", eng.forward(x))
    eng.backward(target=target, ignore_index=-100)
    torch.cuda.synchronize()
    emit(case, "loss_pair", eng._loss)
    for k in sorted(eng.grads):
        emit(case, f"grad.{k}", eng.grads[k])
    eng.close()


def emit_step(case, eng, name="", loss=True):
    import torch
    torch.cuda.synchronize()
    if loss:
        emit(case, f"{name}loss_pair", eng._loss)
    for k in sorted(eng.grads):
        emit(case, f"{name}grad.{k}", eng.grads[k])


def run_train_paths(case, path, backbone="tiny16", S=64, B=2, K=5, group=0, ragged=None, **kw):
    """the paths of the training step run_train does not reach: per-image label lists, the d(logits) hand-over, lseg_train_loss before
    the backward (same target: its pass is reused; another target: it is not), accumulation, the scaled fused loss"""
    import torch
    eng, sd, x = engine(backbone, S, B, K, "bf16", group, **kw)
    eng.enable_training(sd)
    W = kw.get("width") or S
    kout = group if group else K
    gen = torch.Generator().manual_seed(11)
    if ragged:
        eng.set_tokens(eng_tokens(eng, K), group_sizes=ragged)
        target = torch.stack([torch.randint(-1, k, (S, W), generator=torch.Generator().manual_seed(13 + b)) for b, k in enumerate(ragged)]).cuda()
    else:
        target = torch.randint(-1, kout, (B, S, W), generator=gen).cuda()
    if path == "ragged":
        eng.forward(x, want_logits=False)
        emit(case, "train_loss", eng.train_loss(target))
        eng.backward(target=target)
        emit_step(case, eng)
    elif path == "handover":
        logits = eng.forward(x)
        emit(case, "logits", logits)
        eng.backward(dlogits=torch.randn(logits.shape, generator=gen).cuda() * 1e-4)
        emit_step(case, eng, loss=False)
    elif path == "loss_reuse":
        other = torch.randint(-1, kout, (B, S, W), generator=gen).cuda()
        for name, second in (("same.", target), ("other.", other)):
            emit(case, f"{name}logits", eng.forward(x))
            loss, counts = eng.train_loss(target, want_counts=True)
            emit(case, f"{name}train_loss", loss)
            emit(case, f"{name}train_counts", counts)
            eng.backward(target=second)
            emit_step(case, eng, name)
    elif path == "accumulate":
        for name, acc in (("first.", False), ("second.", True)):
            emit(case, f"{name}logits", eng.forward(x))
            eng.backward(target=target, accumulate=acc)
            emit_step(case, eng, name)
    elif path == "grad_scale":
        emit(case, "logits", eng.forward(x))
        eng.backward(target=target, grad_scale=torch.tensor(0.5, device="cuda"))
        emit_step(case, eng, loss=False)
    else:
        raise ValueError(path)
    eng.close()


def run_routes(case, backbone, S, B, K, ragged=None, want=("lowres", "conf", "loss", "features"), **kw):
    """the output tails of Engine::forward that run_eval does not reach (csrc/forward_route.h), each as its own forward of one engine"""
    import torch
    eng, _, x = engine(backbone, S, B, K, "fp16", **kw)
    target = torch.randint(-1, K, (B, S, S), generator=torch.Generator().manual_seed(11)).cuda()

    def emit_dict(name, d):
        for k in sorted(d):
            emit(case, f"{name}.{k}", d[k])

    if "logits" in want:
        emit(case, "logits", eng.forward(x))
    if "lowres" in want:
        emit(case, "forward_lowres", eng.forward_lowres(x))
    if "labels" in want:
        lab, score = eng.forward_labels(x, want_score=True)
        emit(case, "labels", lab)
        emit(case, "score", score)
    if "masks" in want:                                         # K > 256: the int16 fallback of want_argmax
        emit(case, "masks", eng.forward(x, want_logits=False, want_argmax=True))
    if "conf" in want:
        emit_dict("conf", eng.forward_labels_conf(x))
    if "loss" in want:
        emit_dict("loss", eng.forward_labels_loss(x, target))
        emit_dict("loss_plane", eng.forward_labels_loss(x, target, plane=True))
    if "features" in want:
        feat, scale = eng.forward_features(x)
        emit(case, "feat", feat)
        emit(case, "scale", scale)
        half = K // 2
        emit(case, "score_features.0", eng.score_features(feat, scale, 0, half))
        emit(case, "score_features.1", eng.score_features(feat, scale, half, K - half))
    if "stats" in want:                                         # after a logits-only forward: the (2h, 2w) logits are made on demand
        eng.forward(x)
        st = eng.forward_stats(target)
        emit(case, "forward_stats", torch.cat([torch.tensor([st["correct"], st["labeled"], st["nll_count"]]), st["area_inter"], st["area_pred"],
                                               st["area_lab"]]))
        emit(case, "forward_stats.nll", torch.tensor([st["nll_sum"]], dtype=torch.float64))
        if K == 2:
            eng.forward(x)
            emit_dict("episode_stats", eng.episode_stats(target.clamp(min=0), ignore_index=-100))
    if ragged:                                                  # per-image label lists over the same K rows
        eng.set_tokens(eng_tokens(eng, K), group_sizes=ragged)
        tr = torch.stack([torch.randint(-1, k, (S, S), generator=torch.Generator().manual_seed(13 + b)) for b, k in enumerate(ragged)]).cuda()
        lab, score = eng.forward_labels(x, want_score=True)
        emit(case, "ragged.labels", lab)
        emit(case, "ragged.score", score)
        emit_dict("ragged.conf", eng.forward_labels_conf(x))
        emit_dict("ragged.loss", eng.forward_labels_loss(x, tr))
    torch.cuda.synchronize()
    eng.close()


def eng_tokens(eng, K):
    from lseg_hip.synth import synthetic_tokens
    return synthetic_tokens([LABELS[i % len(LABELS)] for i in range(K)], eng.cfg.text.vocab, eng.cfg.text.ctx)


ALL3, TWO = ("fp16", "bf16", "strict"), ("fp16", "bf16")
CASES = {
    # ConvT / identity / conv-s2 resamples, split-K slabs at B = 1, the commuted head, the one-pass x4 upsample, the streamed labels
    "tiny16_b1": lambda c: run_eval(c, "tiny16", 64, 1, 5, ALL3),
    "tiny16_b3": lambda c: run_eval(c, "tiny16", 64, 3, 5, ALL3),
    # the reference-order head, the activation taps
    "tiny16_debug_b1": lambda c: run_eval(c, "tiny16", 64, 1, 5, ALL3, debug=True),
    "tiny16_debug_b3": lambda c: run_eval(c, "tiny16", 64, 3, 5, ALL3, debug=True),
    "tiny32_b2": lambda c: run_eval(c, "tiny32", 96, 2, 7, TWO),
    "tiny16_arch1": lambda c: run_eval(c, "tiny16", 64, 2, 5, TWO, arch_option=1, block_depth=2),
    "tiny16_arch2": lambda c: run_eval(c, "tiny16", 64, 2, 5, TWO, arch_option=2, block_depth=2),
    "tiny16_grouped": lambda c: run_eval(c, "tiny16", 64, 2, 6, TWO, group=3),
    "tiny16_grouped_debug": lambda c: run_eval(c, "tiny16", 64, 2, 6, TWO, group=3, debug=True),
    "tiny16_text_features": lambda c: run_eval(c, "tiny16", 64, 2, 5, TWO, text_features=True),
    "tiny16_corr_generic": lambda c: run_eval(c, "tiny16", 64, 2, 5, TWO),                      # the parent sets LSEG_CORR_GENERIC=1
    "tiny16_train": lambda c: run_train(c, "tiny16", 64, 2, 5),
    "tiny16_train_frozen": lambda c: run_train(c, "tiny16", 64, 2, 5, freeze=True),
    "tiny16_train_grouped": lambda c: run_train(c, "tiny16", 64, 2, 6, group=3),
    "tiny16_train_arch1": lambda c: run_train(c, "tiny16", 64, 2, 5, arch_option=1, block_depth=2, head_block_training=True),
    "rn101_zs": lambda c: run_eval(c, "clip_resnet101", 96, 2, 4, TWO, group=2),
    # real width: the 256-wide tile choices, split_residual
    "vitl16_b1": lambda c: run_eval(c, "clip_vitl16_384", 96, 1, 5, TWO),
    "vitl16_train": lambda c: run_train(c, "clip_vitl16_384", 96, 1, 5),
    # ---- the tails of Engine::forward beyond logits / masks / labels (forward_route.h).  out_c 128 (tiny16): pixel_gram + the generic GEMM
    "tiny16_routes": lambda c: run_routes(c, "tiny16", 64, 2, 5, want=("lowres", "conf", "loss", "features", "stats")),
    "tiny16_episode": lambda c: run_routes(c, "tiny16", 64, 2, 2, want=("stats",)),
    "tiny16_arch1_routes": lambda c: run_routes(c, "tiny16", 64, 2, 5, want=("labels", "lowres"), arch_option=1, block_depth=2),
    "tiny16_no_upsample4x": lambda c: run_eval(c, "tiny16", 64, 2, 5, TWO),                     # the parent sets LSEG_NO_UPSAMPLE4X=1
    "tiny16_corr_fullres": lambda c: run_eval(c, "tiny16", 64, 2, 5, TWO),                      # the parent sets LSEG_CORR_FULLRES=1
    # out_c 512: the dedicated correlation kernel (K <= 157), the streamed labels with confidence and loss, shared set and ragged lists
    "vitl16_routes": lambda c: run_routes(c, "clip_vitl16_384", 96, 2, 5, ragged=[2, 3]),
    "vitl16_k160": lambda c: run_routes(c, "clip_vitl16_384", 96, 1, 160, want=("logits", "lowres", "labels")),     # past corr_planes' LDS
    "vitl16_k300": lambda c: run_routes(c, "clip_vitl16_384", 96, 1, 300, want=("labels", "masks")),               # past uint8
}
CASES.update({
    # ---- the training step's label head (csrc/train_head.h) and the exits of the backward beyond run_train's.  tiny16: out_c 128
    "tiny16_train_ragged": lambda c: run_train_paths(c, "ragged", ragged=[2, 3]),
    "tiny16_train_ragged_gemm": lambda c: run_train_paths(c, "ragged", ragged=[2, 3]),         # the parent sets LSEG_CORR_RAGGED_GEMM=1
    "tiny16_train_handover": lambda c: run_train_paths(c, "handover"),
    "tiny16_train_loss_reuse": lambda c: run_train_paths(c, "loss_reuse"),
    "tiny16_train_accumulate": lambda c: run_train_paths(c, "accumulate"),
    "tiny16_train_grad_scale": lambda c: run_train_paths(c, "grad_scale"),
    "tiny16_train_arch2": lambda c: run_train(c, "tiny16", 64, 2, 5, arch_option=2, block_depth=2, head_block_training=True),
    "tiny16_train_unrounded": lambda c: run_train(c, "tiny16", 64, 2, 5, exact_head_grad=True),
    "tiny16_train_grouped_handover": lambda c: run_train_paths(c, "handover", K=6, group=3),
    # the decoder above the ResNet-101 tower (flags bit 6): the backward stops at the tower outputs
    "rn101_train_decoder": lambda c: run_train(c, "clip_resnet101", 64, 2, 4, group=2, width=96, train_resnet_decoder=True),
})
CHILD_ENV = {"tiny16_train_ragged_gemm": {"LSEG_CORR_RAGGED_GEMM": "1"},
             "tiny16_corr_generic": {"LSEG_CORR_GENERIC": "1"}, "tiny16_no_upsample4x": {"LSEG_NO_UPSAMPLE4X": "1"},
             "tiny16_corr_fullres": {"LSEG_CORR_FULLRES": "1"}}


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--lib", help="the liblseg_hip.so to load (default: the in-tree build)")
    ap.add_argument("--cases", help="comma-separated subset")
    ap.add_argument("--timeout", type=float, default=180.0, help="seconds per child")
    ap.add_argument("--out", help="also write the listing here")
    ap.add_argument("--list", action="store_true")
    ap.add_argument("--child", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.list:
        print("\n".join(CASES))
        return 0
    if a.child:
        import torch
        assert torch.cuda.is_available(), "needs a GPU"
        CASES[a.child](a.child)
        return 0
    names = a.cases.split(",") if a.cases else list(CASES)
    lines = []
    for name in names:
        if name not in CASES:
            print(f"unknown case '{name}'", file=sys.stderr)
            return 2
        env = dict(os.environ, LSEG_SYNTHETIC_TOKENS="1", **CHILD_ENV.get(name, {}))
        if a.lib:                                              # (an older build may lack entry points declared since: none is called here)
            env.update(LSEG_HIP_LIB=os.path.abspath(a.lib), LSEG_HIP_ALLOW_MISSING="1")
        try:
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", name], env=env, stdout=subprocess.PIPE, text=True,
                               timeout=a.timeout)
        except subprocess.TimeoutExpired:
            print(f"case {name}: no result after {a.timeout:.0f} s -- stopping", file=sys.stderr)
            return 124
        sys.stdout.write(r.stdout)
        sys.stdout.flush()
        if r.returncode != 0:
            print(f"case {name}: exit status {r.returncode} -- stopping", file=sys.stderr)
            return r.returncode if r.returncode > 0 else 128 - r.returncode
        lines += r.stdout.splitlines()
    lines.append(f"TOTAL {len(names)} cases {len(lines)} tensors {hashlib.sha256(chr(10).join(lines).encode()).hexdigest()}")
    print(lines[-1])
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
