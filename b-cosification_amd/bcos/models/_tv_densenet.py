"""Plain-PyTorch DenseNet topology with torchvision's module / state-dict names.

The reference builds its B-cosified DenseNet-121 from `torchvision.models.DenseNet` (torchvision==0.17.1:
bcos/models/standard_models.py:2,56-63; bcos/experiments/ImageNet/bcosification/model.py:30-36).  torchvision is
not part of the reference tree (and is absent from the MI355X image), so this file restates the published
topology -- `features` = conv0 / norm0 / relu0 / pool0, denseblock{i} of denselayer{j} (norm1, relu1, conv1 1x1 ->
bn_size * growth, norm2, relu2, conv2 3x3 -> growth; the layer reads the concatenation of everything before it),
transition{i} (norm, relu, conv 1x1 -> C / 2, AvgPool2d(2, 2)), norm5; then `classifier` -- with identical
attribute names, so torchvision checkpoints and B-cosified checkpoints load unchanged.  Nothing B-cos specific
lives here; `bcosify.py` converts the result.  `memory_efficient` is accepted and ignored (the checkpointing branch
recomputes the same values).  If torchvision is installed, standard_models.py uses it instead.
"""
from collections import OrderedDict
from typing import List, Tuple

import torch
import torch.nn as nn
import torch.nn.functional as F
from torch import Tensor


class _DenseLayer(nn.Module):
    def __init__(self, num_input_features: int, growth_rate: int, bn_size: int, drop_rate: float,
                 memory_efficient: bool = False):
        super().__init__()
        self.norm1 = nn.BatchNorm2d(num_input_features)
        self.relu1 = nn.ReLU(inplace=True)
        self.conv1 = nn.Conv2d(num_input_features, bn_size * growth_rate, kernel_size=1, stride=1, bias=False)
        self.norm2 = nn.BatchNorm2d(bn_size * growth_rate)
        self.relu2 = nn.ReLU(inplace=True)
        self.conv2 = nn.Conv2d(bn_size * growth_rate, growth_rate, kernel_size=3, stride=1, padding=1, bias=False)
        self.drop_rate = float(drop_rate)
        self.memory_efficient = memory_efficient

    def bn_function(self, inputs: List[Tensor]) -> Tensor:
        return self.conv1(self.relu1(self.norm1(torch.cat(inputs, 1))))

    def forward(self, input) -> Tensor:
        prev_features = [input] if isinstance(input, Tensor) else input
        new_features = self.conv2(self.relu2(self.norm2(self.bn_function(prev_features))))
        if self.drop_rate > 0:
            new_features = F.dropout(new_features, p=self.drop_rate, training=self.training)
        return new_features


class _DenseBlock(nn.ModuleDict):
    def __init__(self, num_layers: int, num_input_features: int, bn_size: int, growth_rate: int, drop_rate: float,
                 memory_efficient: bool = False):
        super().__init__()
        for i in range(num_layers):
            self.add_module("denselayer%d" % (i + 1),
                            _DenseLayer(num_input_features + i * growth_rate, growth_rate, bn_size, drop_rate, memory_efficient))

    def forward(self, init_features: Tensor) -> Tensor:
        features = [init_features]
        for _, layer in self.items():
            features.append(layer(features))
        return torch.cat(features, 1)


class _Transition(nn.Sequential):
    def __init__(self, num_input_features: int, num_output_features: int):
        super().__init__()
        self.norm = nn.BatchNorm2d(num_input_features)
        self.relu = nn.ReLU(inplace=True)
        self.conv = nn.Conv2d(num_input_features, num_output_features, kernel_size=1, stride=1, bias=False)
        self.pool = nn.AvgPool2d(kernel_size=2, stride=2)


class DenseNet(nn.Module):
    def __init__(self, growth_rate: int = 32, block_config: Tuple[int, ...] = (6, 12, 24, 16), num_init_features: int = 64,
                 bn_size: int = 4, drop_rate: float = 0, num_classes: int = 1000, memory_efficient: bool = False):
        super().__init__()
        self.features = nn.Sequential(OrderedDict([
            ("conv0", nn.Conv2d(3, num_init_features, kernel_size=7, stride=2, padding=3, bias=False)),
            ("norm0", nn.BatchNorm2d(num_init_features)),
            ("relu0", nn.ReLU(inplace=True)),
            ("pool0", nn.MaxPool2d(kernel_size=3, stride=2, padding=1)),
        ]))
        num_features = num_init_features
        for i, num_layers in enumerate(block_config):
            self.features.add_module("denseblock%d" % (i + 1),
                                     _DenseBlock(num_layers, num_features, bn_size, growth_rate, drop_rate, memory_efficient))
            num_features = num_features + num_layers * growth_rate
            if i != len(block_config) - 1:
                self.features.add_module("transition%d" % (i + 1), _Transition(num_features, num_features // 2))
                num_features = num_features // 2
        self.features.add_module("norm5", nn.BatchNorm2d(num_features))
        self.classifier = nn.Linear(num_features, num_classes)
        for m in self.modules():
            if isinstance(m, nn.Conv2d):
                nn.init.kaiming_normal_(m.weight)
            elif isinstance(m, nn.BatchNorm2d):
                nn.init.constant_(m.weight, 1)
                nn.init.constant_(m.bias, 0)
            elif isinstance(m, nn.Linear):
                nn.init.constant_(m.bias, 0)

    def forward(self, x: Tensor) -> Tensor:
        out = F.relu(self.features(x), inplace=True)
        out = torch.flatten(F.adaptive_avg_pool2d(out, (1, 1)), 1)
        return self.classifier(out)
