"""VGG (Simonyan & Zisserman, 2014) — the flagship benchmark model.

Standard configurations; torchvision-compatible layer structure so
parameter counts match the reference's benchmark exactly
(reference benchmark: examples/benchmark/synthetic_benchmark.py uses
torchvision.models vgg16).
"""

from typing import List, Union

import torch
import torch.nn as nn
import torch.nn.functional as F

from ..ops import conv_epilogue, first_conv

_CFGS = {
    "A": [64, "M", 128, "M", 256, 256, "M", 512, 512, "M", 512, 512, "M"],
    "B": [64, 64, "M", 128, 128, "M", 256, 256, "M", 512, 512, "M",
          512, 512, "M"],
    "D": [64, 64, "M", 128, 128, "M", 256, 256, 256, "M", 512, 512, 512,
          "M", 512, 512, 512, "M"],
    "E": [64, 64, "M", 128, 128, "M", 256, 256, 256, 256, "M",
          512, 512, 512, 512, "M", 512, 512, 512, 512, "M"],
}


class VGG(nn.Module):
    def __init__(self, cfg: List[Union[int, str]], num_classes: int = 1000,
                 batch_norm: bool = False, dropout: float = 0.5):
        super().__init__()
        layers: List[nn.Module] = []
        in_ch = 3
        for v in cfg:
            if v == "M":
                layers.append(nn.MaxPool2d(kernel_size=2, stride=2))
            else:
                layers.append(nn.Conv2d(in_ch, v, kernel_size=3, padding=1))
                if batch_norm:
                    layers.append(nn.BatchNorm2d(v))
                layers.append(nn.ReLU(inplace=True))
                in_ch = v
        self.features = nn.Sequential(*layers)
        self.avgpool = nn.AdaptiveAvgPool2d((7, 7))
        self.classifier = nn.Sequential(
            nn.Linear(512 * 7 * 7, 4096),
            nn.ReLU(True),
            nn.Dropout(p=dropout),
            nn.Linear(4096, 4096),
            nn.ReLU(True),
            nn.Dropout(p=dropout),
            nn.Linear(4096, num_classes),
        )

    # The fused epilogue's backward leaves the bias gradient to torch's
    # dx.sum((0, 2, 3)) when set: bitwise the unfused result, one more pass.
    torch_bias_grad = False

    def _features(self, x: torch.Tensor) -> torch.Tensor:
        """``self.features(x)``, with every eligible Conv2d -> ReLU
        [-> MaxPool2d(2, 2)] run as a bias-free convolution plus the fused
        epilogue of ops/conv_epilogue.py. The modules, their parameters
        and the convolution problems stay the same; everything that is not
        eligible calls the modules as they are."""
        if _has_hooks(self.features):
            return self.features(x)
        mods = list(self.features)
        i = 0
        while i < len(mods):
            m = mods[i]
            step = _fusable(mods, i)
            if (step == 2 and not self.torch_bias_grad
                    and first_conv.eligible(x, m)):
                # the image's own stage: convolution, bias and ReLU in one
                # kernel each way (ops/first_conv.py)
                x = first_conv.first_conv_bias_relu(x, m.weight, m.bias)
                i += 2
                continue
            if step:
                pool = step == 3 and conv_epilogue.conv_eligible(x, m, True)
                if pool or conv_epilogue.conv_eligible(x, m, False):
                    x = F.conv2d(x, m.weight, None, m.stride, m.padding,
                                 m.dilation, m.groups)
                    x = conv_epilogue.conv_bias_relu(
                        x, m.bias, pool, self.torch_bias_grad)
                    i += 3 if pool else 2
                    continue
            x = m(x)
            i += 1
        return x

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        x = self._features(x)
        x = self.avgpool(x)
        x = torch.flatten(x, 1)
        return self.classifier(x)


def _has_hooks(m: nn.Module) -> bool:
    return bool(m._forward_hooks or m._forward_pre_hooks
                or m._backward_hooks or m._backward_pre_hooks)


def _fusable(mods, i) -> int:
    """Modules the fused epilogue can take over from ``mods[i]``: 3 for
    Conv2d, ReLU, MaxPool2d(2, 2), 2 for Conv2d, ReLU, 0 for none."""
    if i + 1 >= len(mods):
        return 0
    conv, relu = mods[i], mods[i + 1]
    if type(conv) is not nn.Conv2d or type(relu) is not nn.ReLU:
        return 0
    if _has_hooks(conv) or _has_hooks(relu):
        return 0
    if i + 2 < len(mods):
        p = mods[i + 2]
        if (type(p) is nn.MaxPool2d and not _has_hooks(p)
                and p.kernel_size in (2, (2, 2)) and p.stride in (2, (2, 2))
                and p.padding in (0, (0, 0)) and p.dilation in (1, (1, 1))
                and not p.ceil_mode and not p.return_indices):
            return 3
    return 2


def vgg11(num_classes=1000, batch_norm=False):
    return VGG(_CFGS["A"], num_classes, batch_norm)


def vgg13(num_classes=1000, batch_norm=False):
    return VGG(_CFGS["B"], num_classes, batch_norm)


def vgg16(num_classes=1000, batch_norm=False):
    return VGG(_CFGS["D"], num_classes, batch_norm)


def vgg19(num_classes=1000, batch_norm=False):
    return VGG(_CFGS["E"], num_classes, batch_norm)
