"""Golden vectors of the zero-shot CLIP-ResNet-101 network from the REFERENCE'S OWN CODE (tests/golden/ref_rn101_zs_*.pt).
TEST INFRASTRUCTURE.

Runs the reference's modules/models/lseg_net_zs.py LSegRNNetZS (lseg_vit_zs.py _make_pretrained_clip_rn101 /
_make_resnet_backbone, lseg_blocks_zs.py _make_scratch, the four BN refinenets, head1, the per-image fp16 correlation,
output_conv) on CPU with seeded synthetic weights (lseg_hip.synth, config "clip_resnet101"), through
oracle.make_ref_golden.reference_models() and the stubs of oracle/ref_stubs.  torchvision is not installed and the stub's
`models` is empty: `resnet101` is attached to that module object at run time from tools/tv_resnet_standin.py (a
restatement of torchvision's ResNet-101, tied to transformers.ResNetModel by tests/test_rn101_host.py).

Stored sub-sampled so that every fixture stays well under 1 MiB:
  small  ref_rn101_zs_96x96_b3     fp32 logits, fp16 layer1..4 / path_1 taps, text features, the reference's state-dict keys + shapes
  full   ref_rn101_zs_480x480_b2   fp16 logits at every 4th pixel, sub-sampled fp16 layer1..4 / path_1 taps, text features

    python tools/make_ref_rn101_golden.py
"""
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, ROOT)

from oracle.make_ref_golden import FSS, reference_models        # noqa: E402  (puts oracle/ref_stubs + the package on sys.path)
from lseg_hip.config import get_config                          # noqa: E402
from lseg_hip.synth import read_labels, synthetic_images, synthetic_state_dict   # noqa: E402
import tv_resnet_standin                                        # noqa: E402

# name -> (H, W, class_info, seed, sub-sampling steps {tap: step})
CASES = {
    "ref_rn101_zs_96x96_b3": (96, 96, (4, 0, 9), 31,
                              {"logits": 1, "layer1": 2, "layer2": 2, "layer3": 2, "layer4": 1, "path_1": 8}),
    "ref_rn101_zs_480x480_b2": (480, 480, (2, 7), 32,
                                {"logits": 4, "layer1": 16, "layer2": 8, "layer3": 8, "layer4": 4, "path_1": 16}),
}


def attach_torchvision_standin():
    import torchvision
    torchvision.models.resnet101 = tv_resnet_standin.resnet101


def run_case(H, W, class_info, seed):
    attach_torchvision_standin()
    _, lseg_net_zs = reference_models()
    cfg = get_config("clip_resnet101")
    sd = synthetic_state_dict(cfg, seed=seed)
    names = read_labels(FSS)[:16]
    net = lseg_net_zs.LSegRNNetZS(label_list=names, backbone="clip_resnet101", features=cfg.features, aux=False,
                                  use_pretrained=False, arch_option=0, block_depth=0, activation="lrelu")
    res = net.load_state_dict(sd, strict=False)
    missing = [k for k in res.missing_keys if not k.startswith("clip_pretrained.visual.")]
    unexpected = [k for k in res.unexpected_keys if not k.startswith("clip_pretrained.visual.")]
    assert not missing and not unexpected, (missing[:8], unexpected[:8])
    net.eval()
    taps, tf = {}, []
    for l in range(1, 5):
        getattr(net.pretrained, f"layer{l}").register_forward_hook(
            lambda m, i, o, l=l: taps.__setitem__(f"layer{l}", o.detach().clone()))
    net.scratch.refinenet1.register_forward_hook(lambda m, i, o: taps.__setitem__("path_1", o.detach().clone()))
    enc = net.clip_pretrained.encode_text

    def enc_tap(t):
        f = enc(t)
        tf.append(f.detach().clone())
        return f
    net.clip_pretrained.encode_text = enc_tap
    x = synthetic_images(len(class_info), H, W, seed=seed)
    with torch.no_grad():
        out = net(x, list(class_info))
    tok = torch.cat([net.texts[c] for c in class_info], 0)
    keys = [(k, tuple(v.shape)) for k, v in net.state_dict().items() if not k.startswith("clip_pretrained.visual.")]
    return out, taps, torch.cat(tf, 0), tok, keys


def main():
    gd = os.path.join(ROOT, "tests", "golden")
    only = sys.argv[1:]
    for name, (H, W, ci, seed, sub) in CASES.items():
        if only and name not in only:
            continue
        out, taps, tf, tok, keys = run_case(H, W, ci, seed)
        for t in ("layer1", "layer2", "layer3", "layer4", "path_1"):
            print(f"{name} {t} {tuple(taps[t].shape)} max|x| {taps[t].abs().max().item():.3f}")
        s = sub["logits"]
        logits = out[:, :, ::s, ::s].clone()
        d = {"spec": ("clip_resnet101", H, W, ci, seed), "tokens": tok.clone(), "sub": sub,
             "logits": logits if s == 1 else logits.to(torch.float16),
             "text_features": tf.to(torch.float16).clone(),
             "absmax": {t: float(taps[t].abs().max()) for t in taps}}
        for t in ("layer1", "layer2", "layer3", "layer4", "path_1"):
            k = sub[t]
            d[t] = taps[t][:, :, ::k, ::k].to(torch.float16).clone()
        if s == 1:
            d["state_dict_keys"] = keys
        path = os.path.join(gd, name + ".pt")
        torch.save(d, path)
        print(name, tuple(out.shape), f"{os.path.getsize(path) / 1024:.0f} KiB", "max|logit|", float(out.abs().max()))


if __name__ == "__main__":
    main()
