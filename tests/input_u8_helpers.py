"""Shared by the uint8-input tests: the host statement of the normalisation the uint8 first stages fuse in, and seeded decoded images.

`to_tensor_normalize` is torchvision's ToTensor + Normalize(mean, std) written with the torch calls their sources make
(functional.to_tensor: `img.permute(2, 0, 1).to(float32).div(255)`; functional.normalize: `tensor.sub_(mean).div_(std)` with mean / std as
float32 tensors [3,1,1]) -- torchvision itself is not a dependency of this project.  It runs on the HOST, where that transform runs in
the reference's data loaders (lseg_module.py:37-50): torch's CPU kernels divide (a correctly rounded fp32 division), while its GPU
kernel for a division by a Python scalar multiplies by the reciprocal, which differs in the last bit for some byte values.  The GPU tests
therefore build every float reference input on the host and copy it over.
"""
import numpy as np
import torch

HALF = ((0.5, 0.5, 0.5), (0.5, 0.5, 0.5))                                   # the reference's transform
IMAGENET = ((0.485, 0.456, 0.406), (0.229, 0.224, 0.225))


def to_tensor_normalize(u8_hwc: torch.Tensor, mean, std) -> torch.Tensor:
    """uint8 [..., H, W, 3] on the host -> float32 [..., 3, H, W]"""
    assert u8_hwc.dtype == torch.uint8 and not u8_hwc.is_cuda and u8_hwc.shape[-1] == 3
    x = u8_hwc.movedim(-1, -3).contiguous().to(torch.float32).div(255)
    m = torch.as_tensor(mean, dtype=torch.float32).view(3, 1, 1)
    s = torch.as_tensor(std, dtype=torch.float32).view(3, 1, 1)
    return x.sub_(m).div_(s)


def normalize_table_numpy(mean, std) -> np.ndarray:
    """float32 [3, 256]: the value of every (channel, byte) as three float32 operations -- div, sub, div -- the arithmetic the kernels
    spell out (csrc/input_u8.hip: norm_u8_value)"""
    v = np.arange(256, dtype=np.float32)[None, :]
    m = np.asarray(mean, dtype=np.float32)[:, None]
    s = np.asarray(std, dtype=np.float32)[:, None]
    t = v / np.float32(255.0)
    assert t.dtype == np.float32
    return ((t - m) / s).astype(np.float32)


def images_u8(B: int, H: int, W: int, seed: int, kind: str = "random") -> torch.Tensor:
    """uint8 [B, H, W, 3] on the host.  "arange": every byte value, in an order that puts all 256 values into each channel (the flat
    index times 7 modulo 256: 7 is coprime to 256 and to 3); "random": seeded"""
    n = B * H * W * 3
    if kind == "arange":
        return ((torch.arange(n, dtype=torch.int64) * 7) % 256).to(torch.uint8).view(B, H, W, 3)
    g = torch.Generator().manual_seed(seed)
    return torch.randint(0, 256, (B, H, W, 3), generator=g, dtype=torch.uint8)
