"""Restatement of torchvision's ResNet-101 (torchvision.models.resnet: Bottleneck v1.5 -- the stride sits on the 3x3 conv --,
conv1 7x7/2, bn1, relu, maxpool 3x3/2, layer1..4, avgpool, fc) for the reference-run fixtures.  TEST INFRASTRUCTURE.

torchvision is not installed where the fixtures are made; tools/make_ref_rn101_golden.py attaches `resnet101` from here to the
reference's `torchvision.models` stub at run time.  Same module names and state-dict keys as torchvision, eval-mode forward only.
tests/test_rn101_host.py ties it to an independent implementation (transformers.ResNetModel) on every stage output.
"""
import torch
import torch.nn as nn


def conv3x3(cin, cout, stride=1):
    return nn.Conv2d(cin, cout, kernel_size=3, stride=stride, padding=1, bias=False)


def conv1x1(cin, cout, stride=1):
    return nn.Conv2d(cin, cout, kernel_size=1, stride=stride, bias=False)


class Bottleneck(nn.Module):
    expansion = 4

    def __init__(self, inplanes, planes, stride=1, downsample=None):
        super().__init__()
        self.conv1 = conv1x1(inplanes, planes)
        self.bn1 = nn.BatchNorm2d(planes)
        self.conv2 = conv3x3(planes, planes, stride)
        self.bn2 = nn.BatchNorm2d(planes)
        self.conv3 = conv1x1(planes, planes * self.expansion)
        self.bn3 = nn.BatchNorm2d(planes * self.expansion)
        self.relu = nn.ReLU(inplace=True)
        self.downsample = downsample
        self.stride = stride

    def forward(self, x):
        identity = x
        out = self.relu(self.bn1(self.conv1(x)))
        out = self.relu(self.bn2(self.conv2(out)))
        out = self.bn3(self.conv3(out))
        if self.downsample is not None:
            identity = self.downsample(x)
        return self.relu(out + identity)


class ResNet(nn.Module):
    def __init__(self, layers=(3, 4, 23, 3), num_classes=1000):
        super().__init__()
        self.inplanes = 64
        self.conv1 = nn.Conv2d(3, 64, kernel_size=7, stride=2, padding=3, bias=False)
        self.bn1 = nn.BatchNorm2d(64)
        self.relu = nn.ReLU(inplace=True)
        self.maxpool = nn.MaxPool2d(kernel_size=3, stride=2, padding=1)
        self.layer1 = self._make_layer(64, layers[0])
        self.layer2 = self._make_layer(128, layers[1], stride=2)
        self.layer3 = self._make_layer(256, layers[2], stride=2)
        self.layer4 = self._make_layer(512, layers[3], stride=2)
        self.avgpool = nn.AdaptiveAvgPool2d((1, 1))
        self.fc = nn.Linear(512 * Bottleneck.expansion, num_classes)

    def _make_layer(self, planes, blocks, stride=1):
        downsample = None
        if stride != 1 or self.inplanes != planes * Bottleneck.expansion:
            downsample = nn.Sequential(conv1x1(self.inplanes, planes * Bottleneck.expansion, stride),
                                       nn.BatchNorm2d(planes * Bottleneck.expansion))
        layers = [Bottleneck(self.inplanes, planes, stride, downsample)]
        self.inplanes = planes * Bottleneck.expansion
        layers += [Bottleneck(self.inplanes, planes) for _ in range(1, blocks)]
        return nn.Sequential(*layers)

    def stages(self, x):
        """[layer1 .. layer4] outputs."""
        x = self.maxpool(self.relu(self.bn1(self.conv1(x))))
        out = []
        for layer in (self.layer1, self.layer2, self.layer3, self.layer4):
            x = layer(x)
            out.append(x)
        return out

    def forward(self, x):
        x = self.stages(x)[-1]
        return self.fc(torch.flatten(self.avgpool(x), 1))


def resnet101(pretrained=False, **kwargs):
    """torchvision.models.resnet101 signature; there are no pretrained weights here (the fixtures load synthetic ones)."""
    return ResNet((3, 4, 23, 3), **kwargs)
