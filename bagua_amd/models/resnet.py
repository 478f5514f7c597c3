"""ResNet (He et al., 2015) — used by the async-model-average benchmark
config (BASELINE.json: ResNet-50 + fused SGD)."""

import torch
import torch.nn as nn

from ..contrib.sync_batchnorm import SyncBatchNorm


def _bn_act(bn, relu, x, identity=None):
    """``relu(bn(x))`` or ``relu(bn(x) + identity)``. A SyncBatchNorm takes
    the add and the ReLU into its own kernels (see ``ResNet.fuse_bn_act``);
    every other norm, and a ReLU somebody has hooked, runs as modules."""
    if (ResNet.fuse_bn_act and isinstance(bn, SyncBatchNorm)
            and not (relu._forward_hooks or relu._forward_pre_hooks
                     or relu._backward_hooks or relu._backward_pre_hooks)):
        return bn(x, residual=identity, relu=True)
    out = bn(x)
    if identity is not None:
        out = out + identity
    return relu(out)


class BasicBlock(nn.Module):
    expansion = 1

    def __init__(self, in_planes, planes, stride=1, downsample=None):
        super().__init__()
        self.conv1 = nn.Conv2d(in_planes, planes, 3, stride, 1, bias=False)
        self.bn1 = nn.BatchNorm2d(planes)
        self.relu = nn.ReLU(inplace=True)
        self.conv2 = nn.Conv2d(planes, planes, 3, 1, 1, bias=False)
        self.bn2 = nn.BatchNorm2d(planes)
        self.downsample = downsample

    def forward(self, x):
        identity = x
        out = _bn_act(self.bn1, self.relu, self.conv1(x))
        out = self.conv2(out)
        if self.downsample is not None:
            identity = self.downsample(x)
        return _bn_act(self.bn2, self.relu, out, identity)


class Bottleneck(nn.Module):
    expansion = 4

    def __init__(self, in_planes, planes, stride=1, downsample=None):
        super().__init__()
        self.conv1 = nn.Conv2d(in_planes, planes, 1, bias=False)
        self.bn1 = nn.BatchNorm2d(planes)
        self.conv2 = nn.Conv2d(planes, planes, 3, stride, 1, bias=False)
        self.bn2 = nn.BatchNorm2d(planes)
        self.conv3 = nn.Conv2d(planes, planes * 4, 1, bias=False)
        self.bn3 = nn.BatchNorm2d(planes * 4)
        self.relu = nn.ReLU(inplace=True)
        self.downsample = downsample

    def forward(self, x):
        identity = x
        out = _bn_act(self.bn1, self.relu, self.conv1(x))
        out = _bn_act(self.bn2, self.relu, self.conv2(out))
        out = self.conv3(out)
        if self.downsample is not None:
            identity = self.downsample(x)
        return _bn_act(self.bn3, self.relu, out, identity)


class ResNet(nn.Module):
    # After SyncBatchNorm.convert_sync_batchnorm, every norm that a ReLU
    # follows hands the ReLU, and the residual add in front of it, to the
    # norm's kernels: one rounding after add and ReLU where the modules
    # round three times, and a sign mask kept for backward in place of the
    # activation (kernel path only; elsewhere the choice changes nothing).
    # False runs the modules one by one.
    fuse_bn_act = True

    def __init__(self, block, layers, num_classes=1000):
        super().__init__()
        self.in_planes = 64
        self.conv1 = nn.Conv2d(3, 64, 7, 2, 3, bias=False)
        self.bn1 = nn.BatchNorm2d(64)
        self.relu = nn.ReLU(inplace=True)
        self.maxpool = nn.MaxPool2d(3, 2, 1)
        self.layer1 = self._make_layer(block, 64, layers[0])
        self.layer2 = self._make_layer(block, 128, layers[1], 2)
        self.layer3 = self._make_layer(block, 256, layers[2], 2)
        self.layer4 = self._make_layer(block, 512, layers[3], 2)
        self.avgpool = nn.AdaptiveAvgPool2d((1, 1))
        self.fc = nn.Linear(512 * block.expansion, num_classes)

    def _make_layer(self, block, planes, blocks, stride=1):
        downsample = None
        if stride != 1 or self.in_planes != planes * block.expansion:
            downsample = nn.Sequential(
                nn.Conv2d(self.in_planes, planes * block.expansion, 1,
                          stride, bias=False),
                nn.BatchNorm2d(planes * block.expansion))
        layers = [block(self.in_planes, planes, stride, downsample)]
        self.in_planes = planes * block.expansion
        for _ in range(1, blocks):
            layers.append(block(self.in_planes, planes))
        return nn.Sequential(*layers)

    def forward(self, x):
        x = self.maxpool(_bn_act(self.bn1, self.relu, self.conv1(x)))
        x = self.layer4(self.layer3(self.layer2(self.layer1(x))))
        x = torch.flatten(self.avgpool(x), 1)
        return self.fc(x)


def resnet18(num_classes=1000):
    return ResNet(BasicBlock, [2, 2, 2, 2], num_classes)


def resnet50(num_classes=1000):
    return ResNet(Bottleneck, [3, 4, 6, 3], num_classes)


def resnet101(num_classes=1000):
    return ResNet(Bottleneck, [3, 4, 23, 3], num_classes)


def resnet152(num_classes=1000):
    return ResNet(Bottleneck, [3, 8, 36, 3], num_classes)
