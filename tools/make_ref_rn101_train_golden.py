"""Golden vectors of the CLIP-ResNet-101 zero-shot network's TRAINING step from the REFERENCE'S OWN CODE
(tests/golden/ref_rn101_train_*.pt).  TEST INFRASTRUCTURE; build container only (needs the reference checkout that
oracle/make_ref_golden.py loads).

The reference's LSegRNNetZS (modules/models/lseg_net_zs.py, with the stubs and the torchvision stand-in of
tools/make_ref_rn101_golden.py and the seeded synthetic weights of lseg_hip.synth) is run on CPU:

  1. net.eval(), no_grad: the eval-mode logits of the weights (running-statistics BatchNorm everywhere);
  2. net.train(): ONE forward with batch-statistics BatchNorm in all 104 tower BatchNorms and the refinenets', the criterion of
     LSegmentationModuleZS (tools/make_ref_zs_train_golden.reference_criterion) and one backward().

Recorded (data only): the inputs, class_info, the 0/1 target, the train-mode stage outputs layer_1..4 (sub-sampled, fp16), the
train-mode and eval-mode logits (sub-sampled, fp32), the loss, the gradient of every scratch.* parameter in the packed layout of the
ref_zs_train_* fixtures (norm, sum, first 16 and 64 strided elements), and running_mean / running_var after the step of a spread of
tower BatchNorms (the stem, downsample.1 of layer1 / layer2, bn3 of the last block of every stage, the bn1 / bn2 of a stride-2 block).
The gradients of scratch.* do not depend on whether pretrained.* is differentiated too, so the fixture stays valid for a full tower
backward.

    python tools/make_ref_rn101_train_golden.py
"""
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, ROOT)

from oracle.make_ref_golden import FSS, reference_models        # noqa: E402  (puts oracle/ref_stubs + the package on sys.path)
from oracle.make_ref_train_golden import sample_index           # noqa: E402
from lseg_hip.config import get_config                          # noqa: E402
from lseg_hip.synth import read_labels, synthetic_images, synthetic_state_dict   # noqa: E402
from make_ref_rn101_golden import attach_torchvision_standin    # noqa: E402
from make_ref_zs_train_golden import reference_criterion, zs_target   # noqa: E402

# name -> (H, W, class_info, seed, sub-sampling steps {tap: step}); B = len(class_info).  96 x 96: layer4 is 3 x 3; 64 x 96: non-square,
# layer4 is 2 x 3 (12 samples per channel behind its batch statistics at B = 2)
CASES = {
    "ref_rn101_train_96x96_b3": (96, 96, (4, 0, 9), 61, {"logits": 2, "layer1": 3, "layer2": 3, "layer3": 2, "layer4": 1}),
    "ref_rn101_train_64x96_b2": (64, 96, (7, 2), 62, {"logits": 2, "layer1": 2, "layer2": 2, "layer3": 1, "layer4": 1}),
}
# tower BatchNorms whose running statistics after the step are recorded
BN_SPREAD = ("pretrained.layer1.1", "pretrained.layer1.4.0.downsample.1", "pretrained.layer1.4.2.bn3", "pretrained.layer2.0.downsample.1",
             "pretrained.layer2.0.bn1", "pretrained.layer2.0.bn2", "pretrained.layer2.3.bn3", "pretrained.layer3.11.bn2",
             "pretrained.layer3.22.bn3", "pretrained.layer4.0.bn2", "pretrained.layer4.2.bn3")
N_SAMPLE = 64


def run_case(H, W, class_info, seed):
    attach_torchvision_standin()
    _, lseg_net_zs = reference_models()
    cfg = get_config("clip_resnet101")
    sd = synthetic_state_dict(cfg, seed=seed)
    names = read_labels(FSS)[:16]
    net = lseg_net_zs.LSegRNNetZS(label_list=names, backbone="clip_resnet101", features=cfg.features, aux=False,
                                  use_pretrained=False, arch_option=0, block_depth=0, activation="lrelu")
    res = net.load_state_dict(sd, strict=False)
    assert not [k for k in res.missing_keys + res.unexpected_keys if not k.startswith("clip_pretrained.visual.")]
    B = len(class_info)
    x = synthetic_images(B, H, W, seed=seed)
    target = zs_target(B, H, W, seed)
    net.eval()
    with torch.no_grad():
        eval_logits = net(x, list(class_info)).clone()
    net.train()
    taps = {}
    hooks = [getattr(net.pretrained, f"layer{l}").register_forward_hook(lambda m, i, o, l=l: taps.__setitem__(f"layer{l}", o.detach().clone()))
             for l in range(1, 5)]
    out = net(x, list(class_info))
    loss = reference_criterion(out, target)
    loss.backward()
    for h in hooks:
        h.remove()
    grads = {n: p.grad for n, p in net.named_parameters() if n.startswith("scratch.") and p.grad is not None}
    after = net.state_dict()
    bn = {}
    for p in BN_SPREAD:
        bn[p] = {"running_mean": after[p + ".running_mean"].clone(), "running_var": after[p + ".running_var"].clone(),
                 "num_batches_tracked": int(after[p + ".num_batches_tracked"]),
                 "running_mean_before": sd[p + ".running_mean"].clone(), "running_var_before": sd[p + ".running_var"].clone()}
    tokens = torch.cat([net.texts[c] for c in class_info], 0)
    return x, target, tokens, eval_logits, out.detach(), float(loss), taps, grads, bn


def main():
    gd = os.path.join(ROOT, "tests", "golden")
    only = sys.argv[1:]
    for name, (H, W, ci, seed, sub) in CASES.items():
        if only and name not in only:
            continue
        x, target, tokens, ev, tr, loss, taps, grads, bn = run_case(H, W, ci, seed)
        names = sorted(grads)
        flat = [grads[n].flatten().float() for n in names]
        packed = {"names": names,
                  "norm": torch.tensor([float(f.norm()) for f in flat], dtype=torch.float64),
                  "sum": torch.tensor([float(f.double().sum()) for f in flat], dtype=torch.float64),
                  "n_head": torch.tensor([min(16, f.numel()) for f in flat], dtype=torch.int64),
                  "n_sample": torch.tensor([min(N_SAMPLE, f.numel()) for f in flat], dtype=torch.int64),
                  "values": torch.cat([torch.cat([f[:16], f[sample_index(f.numel(), N_SAMPLE)]]) for f in flat])}
        s = sub["logits"]
        d = {"spec": ("clip_resnet101", H, W, tuple(ci), seed), "class_info": list(ci), "x": x.clone(), "target": target.to(torch.uint8),
             "tokens": tokens.clone(), "sub": sub, "loss": loss, "packed": packed, "bn": bn,
             "train_logits": tr[:, :, ::s, ::s].clone(), "eval_logits": ev[:, :, ::s, ::s].clone()}
        for l in range(1, 5):
            t, k = taps[f"layer{l}"], sub[f"layer{l}"]
            d[f"layer{l}"] = t[:, :, ::k, ::k].to(torch.float16).clone()
            d.setdefault("absmax", {})[f"layer{l}"] = float(t.abs().max())
        path = os.path.join(gd, name + ".pt")
        torch.save(d, path)
        sep = float((tr - ev).pow(2).mean().sqrt() / tr.pow(2).mean().sqrt())
        print(name, "loss", loss, len(names), "scratch gradients; train-vs-eval logits relative rms", round(sep, 4),
              f"{os.path.getsize(path) / 1024:.0f} KiB")


if __name__ == "__main__":
    main()
