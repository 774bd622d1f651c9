"""Plain torch.nn restatement of torchvision's bottleneck ResNet (v1.5: the stride sits on the 3x3) with ``groups`` / ``width_per_group``, written
from the published architecture: conv1, bn1, layer1..4 (blocks conv1/bn1/conv2/bn2/conv3/bn3 [+ downsample.0/.1]), fc -- torchvision's key names.
The reference the ResNet-101 / ResNeXt encoder tests compare against (helper, no tests)."""
import torch
import torch.nn as nn
import torch.nn.functional as F


class Bottleneck(nn.Module):
    expansion = 4

    def __init__(self, inplanes, planes, stride=1, downsample=None, groups=1, base_width=64):
        super().__init__()
        width = int(planes * (base_width / 64.0)) * groups
        self.conv1 = nn.Conv2d(inplanes, width, 1, bias=False)
        self.bn1 = nn.BatchNorm2d(width)
        self.conv2 = nn.Conv2d(width, width, 3, stride, 1, groups=groups, bias=False)
        self.bn2 = nn.BatchNorm2d(width)
        self.conv3 = nn.Conv2d(width, planes * 4, 1, bias=False)
        self.bn3 = nn.BatchNorm2d(planes * 4)
        self.downsample = downsample

    def forward(self, x):
        idt = x if self.downsample is None else self.downsample(x)
        out = F.relu(self.bn1(self.conv1(x)))
        out = F.relu(self.bn2(self.conv2(out)))
        return F.relu(self.bn3(self.conv3(out)) + idt)


class ResNet(nn.Module):
    def __init__(self, layers, groups=1, width_per_group=64, num_classes=1000):
        super().__init__()
        self.inplanes, self.groups, self.base_width = 64, groups, width_per_group
        self.conv1 = nn.Conv2d(3, 64, 7, 2, 3, bias=False)
        self.bn1 = nn.BatchNorm2d(64)
        self.layer1 = self._make_layer(64, layers[0], 1)
        self.layer2 = self._make_layer(128, layers[1], 2)
        self.layer3 = self._make_layer(256, layers[2], 2)
        self.layer4 = self._make_layer(512, layers[3], 2)
        self.fc = nn.Linear(2048, num_classes)
        for m in self.modules():
            if isinstance(m, nn.Conv2d):
                nn.init.kaiming_normal_(m.weight, mode="fan_out", nonlinearity="relu")

    def _make_layer(self, planes, blocks, stride):
        downsample = None
        if stride != 1 or self.inplanes != planes * 4:
            downsample = nn.Sequential(nn.Conv2d(self.inplanes, planes * 4, 1, stride, bias=False), nn.BatchNorm2d(planes * 4))
        layers = [Bottleneck(self.inplanes, planes, stride, downsample, self.groups, self.base_width)]
        self.inplanes = planes * 4
        layers += [Bottleneck(self.inplanes, planes, 1, None, self.groups, self.base_width) for _ in range(1, blocks)]
        return nn.Sequential(*layers)

    def features(self, x):
        """The five maps the depth encoders return: relu(bn1(conv1)), layer1(maxpool), layer2, layer3, layer4 (NCHW)."""
        f0 = F.relu(self.bn1(self.conv1(x)))
        f1 = self.layer1(F.max_pool2d(f0, 3, 2, 1))
        f2 = self.layer2(f1)
        f3 = self.layer3(f2)
        return [f0, f1, f2, f3, self.layer4(f3)]


def resnet101():
    return ResNet([3, 4, 23, 3])


def resnext50_32x4d():
    return ResNet([3, 4, 6, 3], 32, 4)


def resnext101_32x8d():
    return ResNet([3, 4, 23, 3], 32, 8)
