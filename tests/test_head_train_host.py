"""Training with the arch_option 1/2 head blocks, on the host (no GPU): which engines ask for head-block training (lseg_config.flags
bit 4), the bucket of the head-block gradients, and the reference-autograd fixtures tests/golden/ref_head_train_*.pt
(tools/make_ref_head_train_golden.py) against oracle.lseg_oracle.training_step."""
import os
import warnings

import pytest
import torch

from lseg_hip.config import get_config
from lseg_hip.synth import synthetic_state_dict, synthetic_images
from lseg_hip.train import grad_bucket_index
from oracle.lseg_oracle import training_step

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
# the 480 x 480 fixture is a GPU-suite case only (the oracle under autograd at 480 x 480, K = 150 takes minutes of CPU)
SMALL = sorted(f[:-3] for f in os.listdir(GOLD) if f.startswith("ref_head_train_") and "_480x480_" not in f)
HB_KEYS = ("scratch.head_block.depthwise.depthwise.weight", "scratch.head_block.depthwise.depthwise.bias")


class _Recorder:
    """Stands in for lseg_hip.engine.HipEngine: records the keyword arguments LSeg._engine builds an engine with."""
    made = []

    def __init__(self, cfg, H, W, **kw):
        from lseg_hip.engine import to_c_config
        self.max_batch, self.max_labels = kw["max_batch"], kw["max_labels"]
        self.kw = kw
        self.flags = to_c_config(cfg, H, W, kw["max_batch"], kw["max_labels"],
                                 head_block_training=kw.get("head_block_training", False)).flags
        _Recorder.made.append(self)

    def load_state_dict(self, sd):
        pass

    def close(self):
        pass


def _engine_flags(net, monkeypatch):
    import lseg_hip.engine as E
    monkeypatch.setattr(E, "HipEngine", _Recorder)
    _Recorder.made = []
    net._engine(1, 64, 64, 3, torch.device("cpu"), train=True)
    assert len(_Recorder.made) == 1
    return _Recorder.made[0].flags


@pytest.mark.parametrize("arch", [0, 1, 2])
def test_lsegnet_asks_for_head_block_training_exactly_with_head_blocks(arch, monkeypatch):
    warnings.simplefilter("ignore")
    from modules.models.lseg_net import LSegNet
    net = LSegNet(labels=["a", "b", "c"], backbone="tiny16", features=64, arch_option=arch, block_depth=2, activation="lrelu")
    flags = _engine_flags(net, monkeypatch)
    assert bool(flags & 16) == (arch in (1, 2)), flags


def test_lsegnetzs_never_asks_for_head_block_training(monkeypatch):
    warnings.simplefilter("ignore")
    from modules.models.lseg_net_zs import LSegNetZS
    net = LSegNetZS(label_list=["others", "dog"], backbone="tiny16", features=64, arch_option=0, block_depth=0, activation="lrelu")
    assert not _engine_flags(net, monkeypatch) & 16


def test_to_c_config_sets_bit_4_only_on_request():
    from lseg_hip.engine import to_c_config
    cfg = get_config("tiny16", arch_option=1, block_depth=2)
    assert to_c_config(cfg, 64, 64, 1, 3).flags & 16 == 0
    c = to_c_config(cfg, 64, 64, 1, 3, exact_head_grad=True, deterministic=True, head_block_training=True)
    assert c.flags == 2 | 8 | 16


@pytest.mark.parametrize("bb", ["tiny16", "clip_vitl16_384", "clip_vitb32_384"])
def test_head_block_gradients_ride_in_bucket_0(bb):
    cfg = get_config(bb, arch_option=2, block_depth=3)
    for k in HB_KEYS:
        assert grad_bucket_index(k, cfg.depth, cfg.hooks) == 0


def _target(B, H, W, K, seed):          # == oracle/make_ref_train_golden.synthetic_target (importing that module installs the reference stubs)
    g = torch.Generator().manual_seed(1000 + seed)
    t = torch.randint(0, K, (B, H, W), generator=g)
    t[torch.rand((B, H, W), generator=g) < 0.2] = -1
    return t


def _unpack(g):
    p = g["packed"]
    return {n: (float(p["norm"][i]), float(p["sum"][i])) for i, n in enumerate(p["names"])}


def test_there_are_small_head_train_fixtures():
    assert len(SMALL) >= 2 and all(os.path.getsize(os.path.join(GOLD, n + ".pt")) < 1 << 20 for n in SMALL)
    specs = {torch.load(os.path.join(GOLD, n + ".pt"))["spec"][5] for n in SMALL}
    assert specs == {1, 2}                                   # both arch options


@pytest.mark.parametrize("name", SMALL)
def test_oracle_training_step_matches_the_head_train_fixtures(name):
    g = torch.load(os.path.join(GOLD, name + ".pt"))
    bb, H, W, B, K, arch, depth, act, seed = g["spec"]
    cfg = get_config(bb, arch_option=arch, block_depth=depth, activation=act)
    sd = synthetic_state_dict(cfg, seed=seed)
    x = synthetic_images(B, H, W, seed=seed)
    loss, grads = training_step(sd, x, _target(B, H, W, K, seed), g["tokens"], cfg, ignore_index=-1)
    assert abs(float(loss) - g["loss"]) <= 2e-4 * max(1.0, abs(g["loss"]))
    ref = _unpack(g)
    assert set(grads) == set(ref), sorted(set(grads) ^ set(ref))[:8]
    assert all(n not in grads for n in g["no_grad"])
    for k in HB_KEYS:
        assert k in ref and ref[k][0] > 0
    # the bars of tests/test_oracle_train_ref_golden.py at its larger cases: the head blocks (up to three activations on the fp16-valued
    # logits) put the CPU oracle's last-bit differences through more roundings (measured worst 0.30 % on a BatchNorm weight, depth 3 tanh)
    for n, (norm, _) in ref.items():
        tol = 6e-2 if n.startswith("clip_pretrained.") else 6e-3
        err = abs(float(grads[n].float().norm()) - norm) / max(norm, 1e-12)
        assert err <= tol, (n, float(grads[n].norm()), norm)
