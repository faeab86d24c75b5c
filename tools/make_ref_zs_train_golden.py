"""Golden vectors for the ZERO-SHOT training step from the REFERENCE'S OWN CODE (tests/golden/ref_zs_train_*.pt).  TEST INFRASTRUCTURE;
build container only (needs the reference checkout that oracle/make_ref_golden.py loads).

The reference's LSegNetZS (modules/models/lseg_net_zs.py, loaded through oracle.make_ref_golden.reference_models) is put in train()
mode, run on seeded synthetic images with per-image class ids, the loss of LSegmentationModuleZS.training_step is taken with the
reference's criterion (restated below from modules/lsegmentation_module_zs.py:338-343: nn.CrossEntropyLoss() over [B, 2, H*W], torch's
default ignore_index -100) and back-propagated with autograd.  For every parameter the gradient's L2 norm, sum, first 16 and strided
elements are kept -- the content of tests/golden/ref_train_*.pt (oracle/make_ref_train_golden.py) -- plus `class_info`.  The targets are
seeded 0/1 masks (zs_target).

Storage: the per-parameter elements are PACKED into one flat tensor (`packed`: names, norms, sums, sample counts, values; first 16 then
the strided sample of each parameter, in name order, with their counts) -- one storage instead of two small tensors per parameter, whose per-record overhead
is most of a ref_train_*-style file.  The 480 x 480 case stores 512 strided elements per parameter in bf16 (relative rounding 2^-9, far
below the parity bars) to keep the fixture small; the small cases keep fp32 and 64 elements.  tests/test_gpu_train_zs.py unpacks it into
the ref_train_* schema.

The files are named ref_zs_train_* (not ref_train_*): tests/test_gpu_train.py and tests/test_oracle_train_ref_golden.py collect every
ref_train_* fixture as a SHARED-label-set case.

    python tools/make_ref_zs_train_golden.py            # the small cases (seconds)
    python tools/make_ref_zs_train_golden.py --full     # 480 x 480 ViT-L/16, B = 2 (minutes): the head gradient's fp16-subnormal flush
                                                        # depends on the pixel count, so the real size is pinned too
"""
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import oracle.make_ref_golden as M                                               # noqa: E402  (sets up the stand-ins)
from oracle.make_ref_train_golden import sample_index                            # noqa: E402
from lseg_hip.config import get_config                                            # noqa: E402
from lseg_hip.synth import synthetic_state_dict, synthetic_images, read_labels    # noqa: E402

# name -> (backbone, H, W, class_info, seed); B = len(class_info).  The ViT-L case repeats a class and uses class 0.
ZS_TRAIN_CASES = {
    "ref_zs_train_vitl16_64x64_b4": ("clip_vitl16_384", 64, 64, (4, 0, 9, 4), 41),
    "ref_zs_train_vitb32_128x128_b2": ("clip_vitb32_384", 128, 128, (7, 2), 42),
}
ZS_TRAIN_FULL_CASES = {
    "ref_zs_train_vitl16_480x480_b2": ("clip_vitl16_384", 480, 480, (3, 11), 43),
}
N_CLASSES = 16                                    # the first FSS-1000 names (as oracle/make_ref_golden.py's zero-shot cases)


def zs_target(B, H, W, seed):
    """Seeded 0/1 masks ('others' / the class), the layout of a few-shot support / query mask."""
    g = torch.Generator().manual_seed(2000 + seed)
    return torch.randint(0, 2, (B, H, W), generator=g)


def reference_criterion(logit_mask, gt_mask):
    """modules/lsegmentation_module_zs.py:338-343 (LSegmentationModuleZS.criterion with self.cross_entropy_loss = nn.CrossEntropyLoss())."""
    bsz = logit_mask.size(0)
    logit_mask = logit_mask.view(bsz, 2, -1)
    gt_mask = gt_mask.view(bsz, -1).long()
    return torch.nn.CrossEntropyLoss()(logit_mask, gt_mask)


def run_ref_zs_train_case(spec):
    bb, H, W, class_info, seed = spec
    _, lseg_net_zs = M.reference_models()
    cfg = get_config(bb)
    sd = synthetic_state_dict(cfg, seed=seed)
    names = read_labels(M.FSS)[:N_CLASSES]
    net = lseg_net_zs.LSegNetZS(label_list=names, backbone=bb, features=cfg.features, aux=False, use_pretrained=False,
                                arch_option=0, block_depth=0, activation="lrelu")
    M.load_synthetic(net, sd)
    net.train()
    B = len(class_info)
    x = synthetic_images(B, H, W, seed=seed)
    target = zs_target(B, H, W, seed)
    out = net(x, list(class_info))
    loss = reference_criterion(out, target)
    loss.backward()
    grads = {n: p.grad for n, p in net.named_parameters() if p.grad is not None}
    none = sorted(n for n, p in net.named_parameters() if p.grad is None)
    tokens = torch.cat([net.texts[c] for c in class_info], 0)
    return tokens, loss.detach(), grads, none


def main():
    gd = os.path.join(ROOT, "tests", "golden")
    full = "--full" in sys.argv
    cases = ZS_TRAIN_FULL_CASES if full else ZS_TRAIN_CASES
    n_sample, vdt = (512, torch.bfloat16) if full else (64, torch.float32)
    for name, spec in cases.items():
        tokens, loss, grads, none = run_ref_zs_train_case(spec)
        names = sorted(grads)
        flat = [g.flatten().float() for g in (grads[n] for n in names)]
        packed = {"names": names,
                  "norm": torch.tensor([float(f.norm()) for f in flat], dtype=torch.float64),
                  "sum": torch.tensor([float(grads[n].double().sum()) for n in names], dtype=torch.float64),
                  "n_head": torch.tensor([min(16, f.numel()) for f in flat], dtype=torch.int64),
                  "n_sample": torch.tensor([min(n_sample, f.numel()) for f in flat], dtype=torch.int64),
                  "values": torch.cat([torch.cat([f[:16], f[sample_index(f.numel(), n_sample)]]) for f in flat]).to(vdt)}
        bb, H, W, class_info, seed = spec
        path = os.path.join(gd, name + ".pt")
        torch.save({"spec": spec, "class_info": list(class_info), "tokens": tokens, "loss": float(loss), "packed": packed, "no_grad": none}, path)
        print(name, "loss", float(loss), len(names), "gradients;", len(none), "parameters without;", os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
