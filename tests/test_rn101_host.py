"""The zero-shot CLIP-ResNet-101 network on the host (no GPU): the torchvision ResNet-101 restatement the fixtures are made with
(tools/tv_resnet_standin.py) against an independent implementation (transformers.ResNetModel), the module tree / state-dict keys against
the reference's (stored in tests/golden/ref_rn101_zs_96x96_b3.pt), the synthetic weights, the Lightning module and the C config flag."""
import os
import sys
import warnings

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_SMALL = os.path.join(ROOT, "tests", "golden", "ref_rn101_zs_96x96_b3.pt")


def _standin():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    try:
        import tv_resnet_standin
    finally:
        sys.path.pop(0)
    return tv_resnet_standin


def _randomise_bn(model, seed):
    g = torch.Generator().manual_seed(seed)
    for m in model.modules():
        if isinstance(m, torch.nn.BatchNorm2d):
            c = m.num_features
            m.weight.data = 1 + 0.1 * torch.randn(c, generator=g)
            m.bias.data = 0.05 * torch.randn(c, generator=g)
            m.running_mean.data = 0.1 * torch.randn(c, generator=g)
            m.running_var.data = 0.5 + torch.rand(c, generator=g)


def _hf_key(k):
    """torchvision ResNet key -> transformers ResNetModel key."""
    k = k.replace("conv1.weight", "embedder.embedder.convolution.weight", 1) if k.startswith("conv1.") else k
    if k.startswith("bn1."):
        return "embedder.embedder.normalization." + k[4:]
    if k.startswith("layer"):
        stage, j, rest = int(k[5]) - 1, k.split(".")[1], ".".join(k.split(".")[2:])
        p = f"encoder.stages.{stage}.layers.{j}."
        for i, (c, b) in enumerate((("conv1", "bn1"), ("conv2", "bn2"), ("conv3", "bn3"))):
            if rest.startswith(c + "."):
                return p + f"layer.{i}.convolution." + rest[len(c) + 1:]
            if rest.startswith(b + "."):
                return p + f"layer.{i}.normalization." + rest[len(b) + 1:]
        if rest.startswith("downsample.0."):
            return p + "shortcut.convolution." + rest[len("downsample.0."):]
        if rest.startswith("downsample.1."):
            return p + "shortcut.normalization." + rest[len("downsample.1."):]
    return k


def test_torchvision_standin_equals_transformers_resnet():
    """tools/tv_resnet_standin.py (the torchvision ResNet-101 the fixtures run) == transformers.ResNetModel with Bottleneck v1.5
    (downsample_in_bottleneck=False: the stride on the 3x3 conv) on every stage output, after a key-mapped weight copy."""
    transformers = pytest.importorskip("transformers")
    tv = _standin().resnet101().eval()
    _randomise_bn(tv, 0)
    cfg = transformers.ResNetConfig(num_channels=3, embedding_size=64, hidden_sizes=[256, 512, 1024, 2048], depths=[3, 4, 23, 3],
                                    layer_type="bottleneck", hidden_act="relu", downsample_in_first_stage=False,
                                    downsample_in_bottleneck=False)
    hf = transformers.ResNetModel(cfg).eval()
    hsd = hf.state_dict()
    mapped = {}
    for k, v in tv.state_dict().items():
        if k.startswith("fc."):
            continue
        hk = _hf_key(k)
        assert hk in hsd and hsd[hk].shape == v.shape, (k, hk)
        mapped[hk] = v
    assert set(mapped) == set(hsd), sorted(set(hsd) - set(mapped))[:5]
    hf.load_state_dict(mapped)
    x = torch.randn(2, 3, 96, 64, generator=torch.Generator().manual_seed(1))
    with torch.no_grad():
        ours = tv.stages(x)
        theirs = hf(x, output_hidden_states=True).hidden_states[1:]
    assert len(theirs) == 4
    for a, b in zip(ours, theirs):
        assert a.shape == b.shape
        assert ((a - b).abs().max() / b.abs().max()).item() <= 1e-5


def _net(labels):
    from modules.models.lseg_net_zs import LSegRNNetZS
    return LSegRNNetZS(label_list=labels, backbone="clip_resnet101", features=256, aux=False, use_pretrained=False, arch_option=0,
                       block_depth=0, activation="lrelu")


def test_module_tree_matches_the_reference_keys():
    """LSegRNNetZS(label_list=...) has the reference LSegRNNetZS's state-dict keys and shapes (the list stored by the reference run;
    the CLIP visual tower, never run, excluded), and the synthetic weights cover exactly those keys."""
    from lseg_hip.config import get_config
    from lseg_hip.synth import synthetic_state_dict
    ref = dict(torch.load(_SMALL)["state_dict_keys"])
    mine = {k: tuple(v.shape) for k, v in _net(["a", "b"]).state_dict().items() if not k.startswith("clip_pretrained.visual.")}
    assert mine == ref
    assert any(k.startswith("pretrained.layer1.4.") for k in ref) and "pretrained.layer3.22.bn3.weight" in ref
    sd = synthetic_state_dict(get_config("clip_resnet101"), seed=0)
    assert {k: tuple(v.shape) for k, v in sd.items()} == ref


def test_net_surface():
    import torch.nn as nn
    from modules.models.lseg_net_zs import LSegRNNetZS
    with pytest.raises(NotImplementedError):
        LSegRNNetZS()
    net = _net(["cat", "dog", "tree"])
    assert len(net.texts) == 3 and all(tuple(t.shape) == (2, 77) for t in net.texts)
    assert torch.equal(net.texts[0][0], net.texts[2][0])                  # row 0 is always 'others'
    assert net.out_c == 512 and isinstance(net.scratch.head1, nn.Conv2d) and net.cfg.tower == "resnet101"
    assert hasattr(net.scratch.refinenet1.resConfUnit1, "bn1")            # use_bn refinenets
    with pytest.raises(RuntimeError):                                     # no CPU path
        net.eval()(torch.zeros(1, 3, 64, 64), [0])


def test_lightning_module_builds_the_resnet_network():
    warnings.simplefilter("ignore")
    from modules.lseg_module_zs import LSegModuleZS
    from modules.models.lseg_net_zs import LSegRNNetZS
    m = LSegModuleZS("nowhere", "fss", 1, 0.01, 1, backbone="clip_resnet101", num_features=256, arch_option=0, block_depth=0,
                     activation="lrelu", use_pretrained="False", aux=False)
    assert isinstance(m.net, LSegRNNetZS) and m.len_dataloader == 1000 and len(m.net.texts) == 1000
    assert m.net.label_list == m.get_labels("fss")


def test_c_config_selects_the_resnet_tower():
    from lseg_hip.config import get_config
    from lseg_hip.engine import to_c_config
    c = to_c_config(get_config("clip_resnet101"), 480, 480, 4, 8, "fp16")
    assert c.flags & 32 and tuple(c.reassemble_ch) == (256, 512, 1024, 2048)
    assert not to_c_config(get_config("clip_vitl16_384"), 480, 480, 4, 8, "fp16").flags & 32
