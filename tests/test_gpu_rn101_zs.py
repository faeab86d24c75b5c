"""The zero-shot CLIP-ResNet-101 network (LSegRNNetZS, lseg_config.flags bit 5) on the GPU: the ResNet operators (stem, max-pool, 1x1 /
strided convs, the residual-then-ReLU epilogue, whole bottlenecks) against torch fp64 on the same 16-bit operands, and the whole network
against the reference-run fixtures tests/golden/ref_rn101_zs_*.pt (tools/make_ref_rn101_golden.py)."""
import ctypes as C
import math
import os

import pytest
import torch
import torch.nn.functional as F

from lseg_hip import _lib
from lseg_hip.config import get_config
from lseg_hip.engine import HipEngine
from lseg_hip.synth import synthetic_images, synthetic_state_dict

pytestmark = pytest.mark.gpu

DT = {"bf16": (torch.bfloat16, _lib.LSEG_BF16), "fp16": (torch.float16, _lib.LSEG_F16)}
_GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
SMALL, FULL = "ref_rn101_zs_96x96_b3", "ref_rn101_zs_480x480_b2"
# the bars of the ViT networks' fixture tests (tests/test_gpu_forward.py REF_TOL / STAGE_TOL)
REF_TOL = {"bf16": 0.30, "fp16": 0.06}
STAGE_TOL = {"bf16": 0.10, "fp16": 0.015}


@pytest.fixture(scope="module")
def lib():
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    return _lib.load()


def P(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def rnd(shape, seed, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(shape, generator=g) * scale


def pad_nhwc(x_nchw, dtype):
    """NCHW -> padded NHWC (zero border) in the 16-bit type, on the GPU."""
    return F.pad(x_nchw.permute(0, 2, 3, 1), (0, 0, 1, 1, 1, 1)).to(dtype).contiguous().cuda()


def unpad(y_pad):
    return y_pad[:, 1:-1, 1:-1, :].permute(0, 3, 1, 2).double().cpu()


def conv_op(lib, x_pad, w16, bias, res_pad, B, H, W, Cin, Cout, k, s, relu, relu_after, ldt):
    Ho, Wo = (H - 1) // s + 1, (W - 1) // s + 1
    out = torch.zeros((B, Ho + 2, Wo + 2, Cout), dtype=x_pad.dtype, device="cuda")
    wp = (w16.permute(0, 2, 3, 1).reshape(Cout, k * k * Cin) if k == 3 else w16.reshape(Cout, Cin)).contiguous().cuda()
    _lib.check(lib.lseg_op_conv(P(x_pad), P(wp), P(bias), P(res_pad), P(out), B, H, W, Cin, Cout, k, s, int(relu), int(relu_after), ldt,
                                stream()))
    torch.cuda.synchronize()
    return out


def rel_err(a, b):
    return ((a - b).abs().max() / b.abs().max().clamp_min(1e-12)).item()


@pytest.mark.gpu_fast
@pytest.mark.parametrize("dtype", ["bf16", "fp16"])
def test_maxpool_is_bit_exact(lib, dtype):
    tdt, ldt = DT[dtype]
    B, H, W, Cc = 2, 38, 22, 64
    x = torch.relu(rnd((B, Cc, H, W), 1)).to(tdt)
    xp = pad_nhwc(x.float(), tdt)
    out = torch.full((B, H // 2 + 2, W // 2 + 2, Cc), float("nan"), dtype=tdt, device="cuda")
    out[:, 0] = 0; out[:, -1] = 0; out[:, :, 0] = 0; out[:, :, -1] = 0
    _lib.check(lib.lseg_op_rn_maxpool(P(xp), P(out), B, H, W, Cc, ldt, stream()))
    torch.cuda.synchronize()
    ref = F.max_pool2d(x.float(), 3, 2, 1).to(tdt)
    got = out[:, 1:-1, 1:-1, :].permute(0, 3, 1, 2).cpu()
    assert torch.equal(got.view(torch.int16), ref.contiguous().view(torch.int16))
    assert (out[:, 0].float().abs().sum() + out[:, :, 0].float().abs().sum()).item() == 0     # the border stays zero


@pytest.mark.gpu_fast
@pytest.mark.parametrize("dtype", ["bf16", "fp16"])
def test_stem_matches_fp64(lib, dtype):
    tdt, ldt = DT[dtype]
    B, H, W = 2, 64, 96
    x = rnd((B, 3, H, W), 2)
    w = rnd((64, 3, 7, 7), 3, math.sqrt(2 / 147))
    bias = rnd((64,), 4, 0.1)
    wp = w.reshape(64, 147).t().contiguous().cuda()
    out = torch.zeros((B, H // 2 + 2, W // 2 + 2, 64), dtype=tdt, device="cuda")
    xd, bd = x.cuda(), bias.cuda()                  # (kept alive across the launch)
    _lib.check(lib.lseg_op_rn_stem(P(xd), P(wp), P(bd), P(out), B, H, W, ldt, stream()))
    torch.cuda.synchronize()
    ref = torch.relu(F.conv2d(x.double(), w.double(), bias.double(), stride=2, padding=3))
    got = unpad(out)
    ulp = 2 ** -8 if dtype == "bf16" else 2 ** -11                 # the output rounding; fp32 accumulation is far below it
    assert ((got - ref).abs() <= ref.abs() * ulp + 1e-4).all(), (got - ref).abs().max().item()


@pytest.mark.gpu_fast
@pytest.mark.parametrize("dtype", ["bf16", "fp16"])
@pytest.mark.parametrize("k,s,Cin,Cout,H,W", [(1, 1, 64, 256, 24, 20), (1, 2, 256, 512, 24, 20), (3, 2, 128, 128, 24, 20),
                                              (3, 2, 256, 256, 12, 12), (3, 2, 512, 512, 6, 6), (1, 1, 512, 2048, 6, 6)])
def test_conv_1x1_and_strided_match_fp64(lib, dtype, k, s, Cin, Cout, H, W):
    tdt, ldt = DT[dtype]
    B = 2
    x = rnd((B, Cin, H, W), 5).to(tdt)
    w = rnd((Cout, Cin, k, k), 6, 1 / math.sqrt(k * k * Cin)).to(tdt)
    bias = rnd((Cout,), 7, 0.1)
    out = conv_op(lib, pad_nhwc(x.float(), tdt), w, bias.cuda(), None, B, H, W, Cin, Cout, k, s, True, False, ldt)
    ref = torch.relu(F.conv2d(x.double(), w.double(), bias.double(), stride=s, padding=k // 2))
    assert rel_err(unpad(out), ref) < (8e-3 if dtype == "bf16" else 1e-3)


@pytest.mark.gpu_fast
@pytest.mark.parametrize("dtype", ["bf16", "fp16"])
@pytest.mark.parametrize("Cout", [64, 256])          # 64: the generic epilogue, 256: the specialised padded one
def test_relu_after_residual_order(lib, dtype, Cout):
    """relu(conv + b + res) vs relu(conv + b) + res: on inputs where the two differ (a residual of either sign) the flag picks the
    bottleneck's order, and without it the DPT units' order is unchanged."""
    tdt, ldt = DT[dtype]
    B, H, W, Cin = 2, 10, 12, 64
    x = rnd((B, Cin, H, W), 8).to(tdt)
    w = rnd((Cout, Cin, 1, 1), 9, 1 / math.sqrt(Cin)).to(tdt)
    bias = rnd((Cout,), 10, 0.1)
    res = rnd((B, Cout, H, W), 11).to(tdt)
    conv = F.conv2d(x.double(), w.double(), bias.double())
    after = torch.relu(conv + res.double())
    before = torch.relu(conv) + res.double()
    assert (after - before).abs().max().item() > 0.5
    tol = 8e-3 if dtype == "bf16" else 1e-3
    for flag, ref in ((1, after), (0, before)):
        out = conv_op(lib, pad_nhwc(x.float(), tdt), w, bias.cuda(), pad_nhwc(res.float(), tdt), B, H, W, Cin, Cout, 1, 1, True, flag, ldt)
        assert rel_err(unpad(out), ref) < tol, flag


def _bottleneck_ref(x, p, stride, has_ds):
    out = torch.relu(F.conv2d(x, p["w1"], p["b1"]))
    out = torch.relu(F.conv2d(out, p["w2"], p["b2"], stride=stride, padding=1))
    out = F.conv2d(out, p["w3"], p["b3"])
    idn = F.conv2d(x, p["wd"], p["bd"], stride=stride) if has_ds else x
    return torch.relu(out + idn)


@pytest.mark.gpu_fast
@pytest.mark.parametrize("dtype", ["bf16", "fp16"])
@pytest.mark.parametrize("has_ds", [True, False])
def test_bottleneck_block_matches_fp64(lib, dtype, has_ds):
    """One Bottleneck v1.5 through the four operators as the engine strings them (stride 2 + downsample, or the identity block), each
    stage's 16-bit output fed to the next; the fp64 reference runs on the same rounded intermediate inputs."""
    tdt, ldt = DT[dtype]
    B, H, W, wd = 2, 16, 12, 128
    cin, s = (256, 2) if has_ds else (4 * wd, 1)
    x = torch.relu(rnd((B, cin, H, W), 12)).to(tdt)
    p = {"w1": rnd((wd, cin, 1, 1), 13, math.sqrt(2 / cin)), "w2": rnd((wd, wd, 3, 3), 14, math.sqrt(2 / (9 * wd))),
         "w3": rnd((4 * wd, wd, 1, 1), 15, 0.2 / math.sqrt(wd)), "wd": rnd((4 * wd, cin, 1, 1), 16, 1 / math.sqrt(cin))}
    p = {k: v.to(tdt) for k, v in p.items()}
    for i, k in enumerate(("b1", "b2", "b3", "bd")):
        p[k] = rnd((wd if k in ("b1", "b2") else 4 * wd,), 20 + i, 0.1)
    Ho, Wo = H // s, W // s
    xp = pad_nhwc(x.float(), tdt)
    t1 = conv_op(lib, xp, p["w1"], p["b1"].cuda(), None, B, H, W, cin, wd, 1, 1, True, False, ldt)
    t2 = conv_op(lib, t1, p["w2"], p["b2"].cuda(), None, B, H, W, wd, wd, 3, s, True, False, ldt)
    idn = conv_op(lib, xp, p["wd"], p["bd"].cuda(), None, B, H, W, cin, 4 * wd, 1, s, False, False, ldt) if has_ds else xp
    out = conv_op(lib, t2, p["w3"], p["b3"].cuda(), idn, B, Ho, Wo, wd, 4 * wd, 1, 1, True, True, ldt)
    pd = {k: v.double() for k, v in p.items()}
    ref = _bottleneck_ref(x.double(), pd, s, has_ds)
    tol = 3e-2 if dtype == "bf16" else 5e-3                 # three chained 16-bit roundings of the intermediate maps
    assert rel_err(unpad(out), ref) < tol
    # the chained stages one by one on the kernel's own rounded inputs: accumulation-order error only
    r1 = torch.relu(F.conv2d(x.double(), pd["w1"], pd["b1"]))
    assert rel_err(unpad(t1), r1) < (8e-3 if dtype == "bf16" else 1e-3)
    r3 = F.conv2d(unpad(t2), pd["w3"], pd["b3"]) + (unpad(idn) if has_ds else x.double())
    assert rel_err(unpad(out), torch.relu(r3)) < (8e-3 if dtype == "bf16" else 1e-3)


def _tap(eng, name, shape):
    return eng.intermediate(name, shape).float()


def _rel_rms(a, b):
    return ((a - b).pow(2).mean().sqrt() / b.pow(2).mean().sqrt()).item()


def assert_argmax_mismatches_are_ties(out, ref, err, what):
    """Every pixel where the engine's arg-max label differs from the reference's sits where the reference's own top-2 margin is below
    twice the measured logit error (restated from tests/test_gpu_forward.py)."""
    top2 = ref.topk(2, dim=1).values
    margin = top2[:, 0] - top2[:, 1]
    mism = out.argmax(1) != ref.argmax(1)
    worst = margin[mism].max().item() if mism.any() else 0.0
    print(f"{what}: argmax mismatch fraction {mism.float().mean().item():.5f}, max reference margin at a mismatch {worst:.4f}, "
          f"max|dlogit| {err:.4f}")
    assert worst <= 2 * err + 1e-6, (what, worst, err)


def _run_fixture(name, dtype):
    g = torch.load(os.path.join(_GOLD, name + ".pt"))
    bb, H, W, class_info, seed = g["spec"]
    B = len(class_info)
    cfg = get_config(bb)
    sd = synthetic_state_dict(cfg, seed=seed)
    x = synthetic_images(B, H, W, seed=seed)
    eng = HipEngine(cfg, H, W, max_batch=B, max_labels=g["tokens"].shape[0], image_dtype=dtype)
    eng.load_state_dict(sd)
    eng.set_tokens(g["tokens"], labels_per_image=2)
    out = eng.forward(x.cuda())
    torch.cuda.synchronize()
    return g, eng, out, B, H, W


@pytest.mark.parametrize("dtype", ["bf16", "fp16"])
@pytest.mark.parametrize("name", [pytest.param(SMALL, marks=pytest.mark.gpu_fast), FULL])
def test_network_matches_reference_fixtures(name, dtype):
    g, eng, out, B, H, W = _run_fixture(name, dtype)
    sub = g["sub"]
    assert out.shape == (B, 2, H, W) and torch.isfinite(out).all()
    for l in range(4):
        t = f"layer{l + 1}"
        C_, h = 256 << l, H // (4 << l)
        got = _tap(eng, t, (B, C_, h, h * W // H)).cpu()[:, :, ::sub[t], ::sub[t]]
        e = _rel_rms(got, g[t].float())
        print(f"{name} {dtype} {t}: rel rms {e:.4f}")
        assert e <= STAGE_TOL[dtype], (t, e)
    eng.set_debug(True)                              # path_1 exists as a map only off the commuted head (engine.hip)
    x = synthetic_images(B, H, W, seed=g["spec"][4]).cuda()
    dbg = eng.forward(x)
    got = _tap(eng, "path1", (B, 256, H // 2, W // 2)).cpu()[:, :, ::sub["path_1"], ::sub["path_1"]]
    eng.set_debug(False)
    assert (dbg - out).abs().max().item() <= 0.05 * max(1.0, out.abs().max().item())
    e = _rel_rms(got, g["path_1"].float())
    print(f"{name} {dtype} path_1: rel rms {e:.4f}")
    assert e <= STAGE_TOL[dtype], ("path_1", e)
    tf = eng.encode_text().float().cpu()             # the per-image ['others', label] pairs through the CLIP ViT-B/32 text tower
    ref_tf = g["text_features"].float()
    cos = (tf * ref_tf).sum(1) / (tf.norm(dim=1) * ref_tf.norm(dim=1))
    assert cos.min().item() > 0.999, cos
    s = sub["logits"]
    got = out.cpu()[:, :, ::s, ::s]
    ref = g["logits"].float()
    err = (got - ref).abs().max().item()
    print(f"{name} {dtype}: max|dlogit| {err:.4f}")
    assert err <= REF_TOL[dtype]
    assert_argmax_mismatches_are_ties(got, ref, err, f"{name} {dtype}")


def test_refusals():
    cfg = get_config("clip_resnet101")
    with pytest.raises(_lib.LSegError) as e:
        HipEngine(cfg, 64, 64, max_batch=1, max_labels=2, image_dtype="strict")
    assert e.value.code == -5 and "strict" in str(e.value)
    with pytest.raises(_lib.LSegError) as e:
        HipEngine(cfg, 80, 64, max_batch=1, max_labels=2)
    assert e.value.code == -1 and "multiple of 32" in str(e.value)
    eng = HipEngine(cfg, 64, 64, max_batch=1, max_labels=2, image_dtype="bf16")
    rc = eng.lib.lseg_set_train(eng._h, 1)
    assert rc == -5


def test_drop_in_module_equals_engine_bit_for_bit():
    from modules.models.lseg_net_zs import LSegRNNetZS
    names = [f"class{i}" for i in range(10)]
    net = LSegRNNetZS(label_list=names, backbone="clip_resnet101", features=256, aux=False, use_pretrained=False, arch_option=0,
                      block_depth=0, activation="lrelu", image_dtype="fp16")
    sd = synthetic_state_dict(get_config("clip_resnet101"), seed=5)
    net.load_state_dict(sd, strict=False)
    net = net.cuda().eval()
    x = synthetic_images(2, 64, 96, seed=5).cuda()
    ci = [3, 7]
    out = net(x, ci)
    assert out.shape == (2, 2, 64, 96) and out.dtype == torch.float32
    eng = HipEngine(get_config("clip_resnet101"), 64, 96, max_batch=2, max_labels=4, image_dtype="fp16")
    eng.load_state_dict(net.state_dict())
    eng.set_tokens(torch.cat([net.texts[c] for c in ci], 0), labels_per_image=2)
    ref = eng.forward(x)
    torch.cuda.synchronize()
    assert torch.equal(out, ref)
    net.train()
    with pytest.raises(NotImplementedError):
        net(x, ci)
    with torch.no_grad():                         # train() without grad is an inference call, like the reference's eval loop
        assert net(x, ci).shape == (2, 2, 64, 96)


def test_batch_invariant_schedule():
    cfg = get_config("clip_resnet101")
    sd = synthetic_state_dict(cfg, seed=6)
    H = W = 64
    x = synthetic_images(3, H, W, seed=6).cuda()
    from lseg_hip.synth import synthetic_tokens
    tok = synthetic_tokens(["others", "a", "others", "b", "others", "c"])
    eng = HipEngine(cfg, H, W, max_batch=3, max_labels=6, image_dtype="bf16", batch_invariant=True)
    eng.load_state_dict(sd)
    eng.set_tokens(tok, labels_per_image=2)
    full = eng.forward(x)
    eng.set_tokens(tok[2:4], labels_per_image=2)
    one = eng.forward(x[1:2])
    torch.cuda.synchronize()
    assert (full[1] - one[0]).abs().max().item() <= 1e-4 * max(1.0, full.abs().max().item())
