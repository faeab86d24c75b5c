"""Parameter holder for the torchvision ResNet-101 image tower of the zero-shot CLIP-ResNet-101 network.

Same module tree and state-dict keys as the reference's lseg_vit_zs.py _make_pretrained_clip_rn101 / _make_resnet_backbone
(:742-760): `pretrained.layer1 = Sequential(resnet.conv1, resnet.bn1, resnet.relu, resnet.maxpool, resnet.layer1)`,
`pretrained.layer2..4 = resnet.layer2..4`, torchvision's Bottleneck v1.5 (stride on conv2, `downsample = Sequential(1x1 conv, bn)`
on block 0 of every stage).  Parameters only: the forward runs in the HIP engine (lseg_config.flags bit 5).
"""
import torch.nn as nn

from .lseg_vit import _NoForward

RESNET101_LAYERS = (3, 4, 23, 3)


class Bottleneck(_NoForward):
    expansion = 4

    def __init__(self, inplanes, planes, stride=1, downsample=None):
        super().__init__()
        self.conv1 = nn.Conv2d(inplanes, planes, kernel_size=1, bias=False)
        self.bn1 = nn.BatchNorm2d(planes)
        self.conv2 = nn.Conv2d(planes, planes, kernel_size=3, stride=stride, padding=1, bias=False)
        self.bn2 = nn.BatchNorm2d(planes)
        self.conv3 = nn.Conv2d(planes, planes * 4, kernel_size=1, bias=False)
        self.bn3 = nn.BatchNorm2d(planes * 4)
        self.relu = nn.ReLU(inplace=True)
        self.downsample = downsample
        self.stride = stride


def _stage(inplanes, planes, blocks, stride):
    ds = nn.Sequential(nn.Conv2d(inplanes, planes * 4, kernel_size=1, stride=stride, bias=False), nn.BatchNorm2d(planes * 4))
    return nn.Sequential(Bottleneck(inplanes, planes, stride, ds), *[Bottleneck(planes * 4, planes) for _ in range(1, blocks)])


def make_resnet101_backbone() -> nn.Module:
    pretrained = nn.Module()
    pretrained.layer1 = nn.Sequential(nn.Conv2d(3, 64, kernel_size=7, stride=2, padding=3, bias=False), nn.BatchNorm2d(64),
                                      nn.ReLU(inplace=True), nn.MaxPool2d(kernel_size=3, stride=2, padding=1),
                                      _stage(64, 64, RESNET101_LAYERS[0], 1))
    pretrained.layer2 = _stage(256, 128, RESNET101_LAYERS[1], 2)
    pretrained.layer3 = _stage(512, 256, RESNET101_LAYERS[2], 2)
    pretrained.layer4 = _stage(1024, 512, RESNET101_LAYERS[3], 2)
    return pretrained
