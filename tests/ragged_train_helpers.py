"""Shared pieces of the ragged training tests (tests/test_ragged_train_host.py, tests/test_gpu_ragged_train.py): image b of a batch is
scored against its OWN k_b labels, the loss is sum(nll) / sum(valid pixels) over the batch.

  * upsample2x_f64 / ragged_loss_f64 -- a float64 restatement of the loss on per-image low-resolution planes: output_conv's x2 bilinear
    (align_corners=True) written out, log-softmax over the image's own planes, ignore_index.  Differentiable; the host test pins it
    against a per-image F.interpolate + F.cross_entropy loop, the GPU tests take it as their reference.
  * make_planes / make_targets -- the common inputs of the GPU op tests.
  * oracle_ragged_step -- the whole step on the CPU oracle: train-mode tower ONCE for the batch (BatchNorm on batch statistics), then
    each image's features against its own text rows, loss and parameter gradients by autograd.
"""
import torch
import torch.nn.functional as F


def prefix_of(counts):
    p = [0]
    for k in counts:
        p.append(p[-1] + int(k))
    return p


def _taps(n):
    """source taps of the x2 bilinear, align_corners=True: out index i reads i0, i1 with weight l on i1 (float64)"""
    i = torch.arange(2 * n, dtype=torch.float64)
    s = i * (n - 1) / (2 * n - 1)
    i0 = s.floor().clamp(max=n - 1).long()
    i1 = (i0 + 1).clamp(max=n - 1)
    return i0, i1, s - i0.double()


def upsample2x_f64(planes):
    """[k, h, w] float64 -> [k, 2h, 2w]: F.interpolate(scale_factor=2, mode='bilinear', align_corners=True), written out"""
    k, h, w = planes.shape
    y0, y1, ly = _taps(h)
    x0, x1, lx = _taps(w)
    rows = planes[:, y0, :] * (1 - ly)[None, :, None] + planes[:, y1, :] * ly[None, :, None]
    return rows[:, :, x0] * (1 - lx)[None, None, :] + rows[:, :, x1] * lx[None, None, :]


def ragged_loss_f64(planes, target, ignore_index=-100):
    """planes: list of B tensors [k_b, h, w] (any float type, differentiable); target int64 [B, 2h, 2w] with values in [0, k_b) or
    ignore_index (a value outside both contributes nothing, as the kernels treat it).
    Returns (nll_sum, n_valid, lse) -- float64 0-dim tensor, int, list of [2h, 2w] float64 log-sum-exp maps."""
    nll = torch.zeros((), dtype=torch.float64)
    valid = 0
    lses = []
    for b, pl in enumerate(planes):
        z = upsample2x_f64(pl.double())
        lse = torch.logsumexp(z, 0)
        lses.append(lse)
        t = target[b]
        ok = (t != ignore_index) & (t >= 0) & (t < pl.shape[0])
        zt = z.gather(0, t.clamp(0, pl.shape[0] - 1)[None])[0]
        nll = nll + ((lse - zt) * ok).sum()
        valid += int(ok.sum())
    return nll, valid, lses


def make_planes(counts, h, w, seed):
    """fp16-valued fp32 planes like the correlation writes (logits of |z| up to ~14), one tensor [k_b, h, w] per image"""
    g = torch.Generator().manual_seed(seed)
    return [(torch.randn(k, h, w, generator=g) * 4.0).half().float() for k in counts]


def make_targets(counts, H, W, seed, ignore_index=-100, ignored_image=None):
    """int64 [B, H, W], uniform in [0, k_b) with about 10 % ignore_index; ignored_image: that image entirely ignored.  The ignore MASK
    depends on (H, W, seed) only, so batches with other counts share it (and with it the number of valid pixels)."""
    g = torch.Generator().manual_seed(seed)
    B = len(counts)
    mask = torch.rand(B, H, W, generator=g) < 0.1
    u = torch.rand(B, H, W, generator=g)
    t = torch.stack([(u[b] * counts[b]).long().clamp(max=counts[b] - 1) for b in range(B)])
    t[mask] = ignore_index
    if ignored_image is not None:
        t[ignored_image] = ignore_index
    return t


def ragged_rows_reference(planes, target, ldk, ignore_index=-100):
    """float64 autograd through ragged_loss_f64: (loss, lse list, d loss / d planes as rows [B*h*w, ldk], zeros beyond k_b)"""
    leaves = [p.double().clone().requires_grad_(True) for p in planes]
    nll, valid, lses = ragged_loss_f64(leaves, target, ignore_index)
    loss = nll / valid
    loss.backward()
    h, w = planes[0].shape[1:]
    rows = torch.zeros(len(planes) * h * w, ldk, dtype=torch.float64)
    for b, p in enumerate(leaves):
        rows[b * h * w:(b + 1) * h * w, :p.shape[0]] = p.grad.reshape(p.shape[0], h * w).t()
    return float(loss.detach()), float(nll.detach()), valid, [l.detach() for l in lses], rows


def oracle_ragged_step(sd, x, target, tok, counts, cfg, ignore_index=-100):
    """Loss and parameter gradients of the ragged step on the CPU oracle: ONE train-mode forward of the image tower over the batch
    (oracle.lseg_forward(bn_train=True): BatchNorm on the batch's statistics), then image b's pixel features against its own text rows
    (oracle.correlate, the fp16 rounding points of lseg_net.py:191-196), x2 bilinear, cross-entropy summed over the batch and divided by
    the batch's valid pixels.  The text tower is frozen (no leaf)."""
    from oracle.lseg_oracle import correlate, lseg_forward
    bn_stats = ("running_mean", "running_var", "num_batches_tracked")
    leaves = {k: v.detach().clone().requires_grad_(True) for k, v in sd.items()
              if v.is_floating_point() and not k.endswith(bn_stats) and not k.startswith("clip_pretrained.")}
    full = dict(sd)
    full.update(leaves)
    _, inter = lseg_forward(full, x, tok, cfg, bn_train=True, return_intermediates=True)
    feat, text = inter["image_features"], inter["text_features"].detach()
    B, Cc, h, w = feat.shape
    imf = feat.permute(0, 2, 3, 1).reshape(B, h * w, Cc)
    pre = prefix_of(counts)
    nll, valid = 0.0, 0
    for b in range(B):
        low = correlate(imf[b], text[pre[b]:pre[b + 1]]).view(1, h, w, -1).permute(0, 3, 1, 2)
        out = F.interpolate(low, scale_factor=2, mode="bilinear", align_corners=True)
        nll = nll + F.cross_entropy(out, target[b:b + 1], ignore_index=ignore_index, reduction="sum")
        valid += int((target[b] != ignore_index).sum())
    loss = nll / valid
    loss.backward()
    return float(loss.detach()), {k: v.grad for k, v in leaves.items() if v.grad is not None}
