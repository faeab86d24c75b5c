"""Golden vectors for the training step WITH arch_option 1/2 HEAD BLOCKS from the REFERENCE'S OWN CODE (tests/golden/ref_head_train_*.pt).
TEST INFRASTRUCTURE; build container only (needs the reference checkout that oracle/make_ref_golden.py loads).

The reference's LSegNet(arch_option, block_depth, activation) (modules/models/lseg_net.py, loaded through
oracle.make_ref_golden.reference_models) is put in train() mode, run on seeded synthetic images, the loss of
LSegmentationModule.training_step (CrossEntropyLoss(ignore_index=-1), as oracle/make_ref_train_golden.py) is back-propagated with
autograd -- through scratch.head_block applied max(block_depth - 1, 0) + 1 times (lseg_net.py:198-201) -- and for every parameter the
gradient's L2 norm, sum, first 16 and strided elements are kept, PACKED into one flat tensor as tools/make_ref_zs_train_golden.py does.
The targets and the strided sample are oracle/make_ref_train_golden.py's (synthetic_target, sample_index).

The files are named ref_head_train_* (not ref_train_*): tests/test_gpu_train.py and tests/test_oracle_train_ref_golden.py collect every
ref_train_* fixture as an arch_option 0 case.

    python tools/make_ref_head_train_golden.py          # the small cases (seconds)
    python tools/make_ref_head_train_golden.py --full   # 480 x 480 ViT-L/16, K = 150, B = 2 (minutes): the fp16-subnormal head gradient at
                                                        # the real pixel count, 512 bf16 strided samples per gradient
"""
import os
import sys

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import oracle.make_ref_golden as M                                               # noqa: E402  (sets up the stand-ins)
from oracle.make_ref_train_golden import sample_index, synthetic_target          # noqa: E402
from lseg_hip.config import get_config                                            # noqa: E402
from lseg_hip.synth import synthetic_state_dict, synthetic_images, read_labels    # noqa: E402

# name -> (backbone, H, W, B, K, arch_option, block_depth, activation, seed)
HEAD_TRAIN_CASES = {
    "ref_head_train_vitl16_64x64_k5_b2_arch1_d2_lrelu": ("clip_vitl16_384", 64, 64, 2, 5, 1, 2, "lrelu", 51),
    "ref_head_train_vitb32_128x128_k4_b2_arch2_d3_tanh": ("clip_vitb32_384", 128, 128, 2, 4, 2, 3, "tanh", 52),
}
HEAD_TRAIN_FULL_CASES = {
    "ref_head_train_vitl16_480x480_k150_b2_arch1_d2_relu": ("clip_vitl16_384", 480, 480, 2, 150, 1, 2, "relu", 53),
}


def case_config(spec):
    bb, H, W, B, K, arch, depth, act, seed = spec
    return get_config(bb, arch_option=arch, block_depth=depth, activation=act)


def run_ref_head_train_case(spec):
    bb, H, W, B, K, arch, depth, act, seed = spec
    lseg_net, _ = M.reference_models()
    cfg = case_config(spec)
    sd = synthetic_state_dict(cfg, seed=seed)
    net = lseg_net.LSegNet(labels=read_labels(M.LABELS)[:K], backbone=bb, features=cfg.features, crop_size=H,
                           arch_option=arch, block_depth=depth, activation=act)
    M.load_synthetic(net, sd)
    net.train()
    x = synthetic_images(B, H, W, seed=seed)
    target = synthetic_target(B, H, W, K, seed)
    out = net(x)
    loss = F.cross_entropy(out, target, ignore_index=-1)
    loss.backward()
    grads = {n: p.grad for n, p in net.named_parameters() if p.grad is not None}
    none = sorted(n for n, p in net.named_parameters() if p.grad is None)
    return net.text.clone(), loss.detach(), grads, none


def main():
    gd = os.path.join(ROOT, "tests", "golden")
    full = "--full" in sys.argv
    cases = HEAD_TRAIN_FULL_CASES if full else HEAD_TRAIN_CASES
    n_sample, vdt = (512, torch.bfloat16) if full else (64, torch.float32)
    for name, spec in cases.items():
        tokens, loss, grads, none = run_ref_head_train_case(spec)
        names = sorted(grads)
        flat = [g.flatten().float() for g in (grads[n] for n in names)]
        packed = {"names": names,
                  "norm": torch.tensor([float(f.norm()) for f in flat], dtype=torch.float64),
                  "sum": torch.tensor([float(grads[n].double().sum()) for n in names], dtype=torch.float64),
                  "n_head": torch.tensor([min(16, f.numel()) for f in flat], dtype=torch.int64),
                  "n_sample": torch.tensor([min(n_sample, f.numel()) for f in flat], dtype=torch.int64),
                  "values": torch.cat([torch.cat([f[:16], f[sample_index(f.numel(), n_sample)]]) for f in flat]).to(vdt)}
        path = os.path.join(gd, name + ".pt")
        torch.save({"spec": spec, "tokens": tokens, "loss": float(loss), "packed": packed, "no_grad": none}, path)
        print(name, "loss", float(loss), len(names), "gradients;", len(none), "parameters without;", os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
