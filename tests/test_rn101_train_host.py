"""Host side of the opt-in decoder training of the CLIP-ResNet-101 zero-shot network (LSegRNNetZS(train_decoder=True), lseg_config.flags
bit 6): the kwarg travels module -> network -> engine config, the optimizer groups are the reference's, a default network still raises
under train(), and the reference-run fixtures of tools/make_ref_rn101_train_golden.py carry what tests/test_gpu_rn101_train_decoder.py
reads.  No GPU."""
import os
import warnings

import pytest
import torch

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
FIXTURES = {"ref_rn101_train_96x96_b3": (96, 96, 3), "ref_rn101_train_64x96_b2": (64, 96, 2)}


def _module(**kw):
    warnings.simplefilter("ignore")
    from modules.lseg_module_zs import LSegModuleZS
    return LSegModuleZS("nowhere", "fss", 2, 0.004, 10, backbone="clip_resnet101", num_features=256, arch_option=0, block_depth=0,
                        activation="lrelu", use_pretrained="False", aux=False, weight_decay=1e-4, **kw)


@pytest.fixture(scope="module")
def opt_in():
    return _module(train_decoder=True)


class _RecordingEngine:
    """Stands in for lseg_hip.engine.HipEngine: keeps the constructor's keyword arguments, does nothing else."""
    made = []

    def __init__(self, cfg, H, W, max_batch, max_labels, device=None, **kw):
        self.cfg, self.max_batch, self.max_labels, self.kw = cfg, max_batch, max_labels, kw
        self.train_resnet_decoder = bool(kw.get("train_resnet_decoder", False))
        self.training, self.grads, self.grad_buckets = False, {}, []
        type(self).made.append(self)

    def load_state_dict(self, sd):
        pass

    def enable_training(self, sd, freeze_encoder=False):
        self.training = True

    def set_train(self, on):
        self.training = bool(on)

    def close(self):
        pass


def test_the_kwarg_reaches_the_engine_config_flag(opt_in, monkeypatch):
    import lseg_hip.engine as E
    from lseg_hip.config import get_config
    cfg = get_config("clip_resnet101")
    assert E.to_c_config(cfg, 96, 96, 2, 4, "bf16", train_resnet_decoder=True).flags & 64
    assert not E.to_c_config(cfg, 96, 96, 2, 4, "bf16").flags & 64
    assert opt_in.net.train_decoder is True
    assert _module().net.train_decoder is False
    monkeypatch.setattr(E, "HipEngine", _RecordingEngine)
    _RecordingEngine.made.clear()
    dev = torch.device("cpu")
    eng = opt_in.net._train_engine(2, 96, 96, 4, dev)
    assert eng.kw["train_resnet_decoder"] is True and eng.kw["image_dtype"] == "bf16"
    # every BatchNorm of the tower counts its batches in train() mode, as the refinenets' do
    nbt = {k for k, b in opt_in.net.named_buffers() if any(b is t for t in eng._nbt)}
    assert "pretrained.layer1.1.num_batches_tracked" in nbt and "pretrained.layer3.22.bn3.num_batches_tracked" in nbt
    assert "scratch.refinenet1.resConfUnit1.bn1.num_batches_tracked" in nbt
    assert len([k for k in nbt if k.startswith("pretrained.")]) == 104
    # the inference engine of the same network is built without the flag
    ev = opt_in.net._engine(2, 96, 96, 4, dev, train=False)
    assert ev.kw["train_resnet_decoder"] is False
    opt_in.net._engines.clear()


def test_optimizer_groups_are_the_reference_groups(opt_in):
    (opt,), (sch,) = opt_in.configure_optimizers()
    net = opt_in.net
    lr = 0.004 / 16 * 2
    g = opt.param_groups
    assert len(g) == 3                                                    # pretrained, scratch, the (empty) auxlayer group
    assert [x["lr"] for x in g] == pytest.approx([lr, 10 * lr, 10 * lr])
    assert {id(p) for p in g[0]["params"]} == {id(p) for p in net.pretrained.parameters()}
    assert {id(p) for p in g[1]["params"]} == {id(p) for p in net.scratch.parameters()}
    assert len(g[2]["params"]) == 0
    assert all(x["momentum"] == 0.9 and x["weight_decay"] == 1e-4 for x in g)
    from modules.lsegmentation_module import EngineAdam, EngineSGD
    assert isinstance(opt, EngineSGD)
    (adam,), _ = _module(train_decoder=True, midasproto=True).configure_optimizers()
    assert isinstance(adam, EngineAdam) and len(adam.param_groups) == 3


def test_fused_step_accepts_the_inert_pretrained_group(opt_in):
    """The engine holds gradients for scratch.* only; the pretrained group of the reference's layout is in the optimizer with .grad None.
    _groups_match must accept that on a decoder-only engine and nowhere else."""
    (opt,), _ = opt_in.configure_optimizers()
    net = opt_in.net
    eng = _RecordingEngine(net.cfg, 96, 96, 2, 4, train_resnet_decoder=True)
    eng.grads = {k: None for k, _ in net.named_parameters() if k.startswith("scratch.") and ".refinenet4.resConfUnit1." not in k}
    assert opt._fusable(eng)
    plain = _RecordingEngine(net.cfg, 96, 96, 2, 4)
    plain.grads = dict(eng.grads)
    opt._fusable_cache = (None, None)
    assert not opt._fusable(plain)


def test_default_network_still_raises_under_train():
    net = _module().net
    net.train()
    with pytest.raises(NotImplementedError, match="inference only"):
        net(torch.zeros(1, 3, 64, 64), [0])
    with pytest.raises(NotImplementedError, match="inference only"):
        net.forward_loss(torch.zeros(1, 3, 64, 64), [0], torch.zeros(1, 64, 64, dtype=torch.long))


def test_data_parallel_trainer_refuses_sync_bn_on_the_tower():
    from lseg_hip.train import DataParallelTrainer
    eng = _RecordingEngine(None, 96, 96, 2, 4, train_resnet_decoder=True)
    with pytest.raises(NotImplementedError, match="ResNet-101 tower"):
        DataParallelTrainer(eng, {}, sync_bn=True)


@pytest.mark.parametrize("name", sorted(FIXTURES))
def test_fixture_files_carry_the_recorded_fields(name):
    H, W, B = FIXTURES[name]
    path = os.path.join(GOLD, name + ".pt")
    assert os.path.getsize(path) < (1 << 20)
    g = torch.load(path)
    assert g["spec"][:3] == ("clip_resnet101", H, W) and len(g["class_info"]) == B
    assert g["x"].shape == (B, 3, H, W) and g["x"].dtype == torch.float32
    assert g["target"].shape == (B, H, W) and set(g["target"].unique().tolist()) <= {0, 1}
    assert g["tokens"].shape == (2 * B, 77)
    s = g["sub"]
    for l in range(4):
        C, h, w = 256 << l, H >> (2 + l), W >> (2 + l)
        k = s[f"layer{l + 1}"]
        assert g[f"layer{l + 1}"].shape == (B, C, -(-h // k), -(-w // k)), (l, g[f"layer{l + 1}"].shape)
    k = s["logits"]
    assert g["train_logits"].shape == g["eval_logits"].shape == (B, 2, H // k, W // k)
    # batch statistics are not running statistics: the two sets of logits differ by far more than any 16-bit tower error
    sep = ((g["train_logits"] - g["eval_logits"]).pow(2).mean().sqrt() / g["train_logits"].pow(2).mean().sqrt()).item()
    assert sep > 0.2, sep
    assert 0.3 < g["loss"] < 2.0
    p = g["packed"]
    assert all(n.startswith("scratch.") for n in p["names"]) and len(p["names"]) == 56
    assert "scratch.layer4_rn.weight" in p["names"] and "scratch.head1.bias" in p["names"]
    assert not [n for n in p["names"] if ".refinenet4.resConfUnit1." in n]
    assert int((p["n_head"] + p["n_sample"]).sum()) == p["values"].numel() and bool((p["norm"] > 0).all())
    bn = g["bn"]
    assert "pretrained.layer1.1" in bn and any(k.endswith("downsample.1") for k in bn)
    for l in range(1, 5):
        assert any(k.startswith(f"pretrained.layer{l}.") and k.endswith("bn3") for k in bn), l
    for k, v in bn.items():
        assert v["num_batches_tracked"] >= 1 and v["running_mean"].shape == v["running_var"].shape == v["running_mean_before"].shape
        assert not torch.equal(v["running_mean"], v["running_mean_before"]), k
