"""B-cos ConvNeXt topology (Liu et al., "A ConvNet for the 2020s") with the reference's module and state-dict names
(bcos/models/convnext.py:32-219): `features.0` the 4x4 stride-4 stem conv, `features.1` its position norm, then per stage a
Sequential of `CNBlock`s (`features.K.J.block.{0,1,2,3}`, `features.K.J.layer_scale`) followed, except behind the last stage, by a
downsampling Sequential (`features.K.0` position norm, `features.K.1` 2x2 stride-2 conv); `classifier.{0,1}` (position norm, 1x1 conv to
the classes) runs BEFORE the global average pool (:202-208), then the LogitLayer.

A block (:45-65) is: depthwise 7x7 B-cos conv -> position norm -> 1x1 B-cos conv to 4 dim -> 1x1 B-cos conv back to dim (no GELU: the
B-cos transform is the non-linearity), times `layer_scale`, stochastic depth, plus the block input.  The depthwise layer is the one
piece with a kernel of its own (csrc/bcos_dwconv.hip, routed by BcosConv2d); the norms are DetachablePositionNorm2d without bias.
Every block opts its depthwise layer in to the training-mode gradients (csrc/bcos_dwconv_train.hip), so `net.train(); net(x);
loss.backward()` trains a BcosConvNeXt per layer like the reference; a bare depthwise BcosConv2d still refuses them.

torchvision is not part of this package's requirements, so `StochasticDepth` ("row" mode, torchvision.ops.StochasticDepth) is restated
here: the identity in eval mode or at p = 0.
"""
import math
from functools import partial
from typing import Any, Callable, List, Optional, Sequence

import torch
from torch import Tensor, nn

from bcos.common import BcosUtilMixin
from bcos.modules import BcosConv2d, LogitLayer, norms
from bcos.modules._hipfn import conv_is_depthwise7

__all__ = ["BcosConvNeXt", "convnext_atto", "convnext_tiny", "convnext_small", "convnext_base", "convnext_large", "CNBlock",
           "CNBlockConfig", "StochasticDepth"]

DEFAULT_NORM_LAYER = norms.NoBias(norms.DetachablePositionNorm2d)
DEFAULT_CONV_LAYER = BcosConv2d


class StochasticDepth(nn.Module):
    """Drops the residual branch of whole samples with probability p while training and rescales the survivors by 1 / (1 - p)
    ("row" mode), or of the whole batch at once ("batch" mode); the identity in eval mode or at p = 0."""

    def __init__(self, p: float, mode: str) -> None:
        super().__init__()
        if p < 0.0 or p > 1.0:
            raise ValueError(f"drop probability has to be between 0 and 1, but got {p}")
        if mode not in ("batch", "row"):
            raise ValueError(f"mode has to be either 'batch' or 'row', but got {mode}")
        self.p, self.mode = p, mode

    def forward(self, x: Tensor) -> Tensor:
        if not self.training or self.p == 0.0:
            return x
        survival = 1.0 - self.p
        shape = [x.shape[0]] + [1] * (x.dim() - 1) if self.mode == "row" else [1] * x.dim()
        keep = torch.empty(shape, dtype=x.dtype, device=x.device).bernoulli_(survival)
        if survival > 0.0:
            keep.div_(survival)
        return x * keep

    def extra_repr(self) -> str:
        return f"p={self.p}, mode={self.mode}"


class CNBlock(nn.Module):
    """One ConvNeXt block (reference :32-65)."""

    def __init__(self, dim, layer_scale: float, stochastic_depth_prob: float, conv_layer: Callable[..., nn.Module] = DEFAULT_CONV_LAYER,
                 norm_layer: Optional[Callable[..., nn.Module]] = DEFAULT_NORM_LAYER) -> None:
        super().__init__()
        if norm_layer is None:
            norm_layer = partial(DEFAULT_NORM_LAYER, eps=1e-6)
        self.block = nn.Sequential(
            conv_layer(dim, dim, kernel_size=7, padding=3, groups=dim, bias=False),
            norm_layer(dim),
            conv_layer(in_channels=dim, out_channels=4 * dim, kernel_size=1, bias=False),
            conv_layer(in_channels=4 * dim, out_channels=dim, kernel_size=1, bias=False),
        )
        dw = self.block[0]
        if isinstance(dw, BcosConv2d) and conv_is_depthwise7(dw.linear, dw.max_out):
            dw.enable_depthwise_training()          # the training-mode gradients of csrc/bcos_dwconv_train.hip
        self.layer_scale = nn.Parameter(torch.ones(dim, 1, 1) * layer_scale)
        self.stochastic_depth = StochasticDepth(stochastic_depth_prob, "row")

    def forward(self, input: Tensor) -> Tensor:
        result = self.layer_scale * self.block(input)
        result = self.stochastic_depth(result)
        result += input
        return result


class CNBlockConfig:
    """(input channels, channels behind the stage's downsampling or None for the last stage, number of blocks) of one stage."""

    def __init__(self, input_channels: int, out_channels: Optional[int], num_layers: int) -> None:
        self.input_channels = input_channels
        self.out_channels = out_channels
        self.num_layers = num_layers

    def __repr__(self) -> str:
        return (f"{self.__class__.__name__}(input_channels={self.input_channels}, out_channels={self.out_channels}, "
                f"num_layers={self.num_layers})")


class BcosConvNeXt(BcosUtilMixin, nn.Module):
    """Constructor arguments and defaults are the reference's (:90-103)."""

    def __init__(self, block_setting: List[CNBlockConfig], stochastic_depth_prob: float = 0.0, layer_scale: float = 1e-6,
                 num_classes: int = 1000, in_chans: int = 6, block: Optional[Callable[..., nn.Module]] = None,
                 conv_layer: Callable[..., nn.Module] = DEFAULT_CONV_LAYER, norm_layer: Optional[Callable[..., nn.Module]] = None,
                 logit_bias: Optional[float] = None, logit_temperature: Optional[float] = None, **kwargs: Any) -> None:
        super().__init__()
        if not block_setting:
            raise ValueError("The block_setting should not be empty")
        if not (isinstance(block_setting, Sequence) and all(isinstance(s, CNBlockConfig) for s in block_setting)):
            raise TypeError("The block_setting should be List[CNBlockConfig]")
        if block is None:
            block = CNBlock
        if norm_layer is None:
            norm_layer = partial(DEFAULT_NORM_LAYER, eps=1e-6)

        stem_channels = block_setting[0].input_channels
        layers: List[nn.Module] = [conv_layer(in_chans, stem_channels, kernel_size=4, stride=4, padding=0, bias=False),
                                   norm_layer(stem_channels)]
        total_blocks = sum(cnf.num_layers for cnf in block_setting)
        block_id = 0
        for cnf in block_setting:
            stage: List[nn.Module] = []
            for _ in range(cnf.num_layers):
                # the drop probability grows linearly with the depth of the block (:146-148)
                sd_prob = stochastic_depth_prob * block_id / (total_blocks - 1.0)
                stage.append(block(cnf.input_channels, layer_scale, sd_prob, conv_layer=conv_layer, norm_layer=norm_layer))
                block_id += 1
            layers.append(nn.Sequential(*stage))
            if cnf.out_channels is not None:
                layers.append(nn.Sequential(norm_layer(cnf.input_channels),
                                            conv_layer(cnf.input_channels, cnf.out_channels, kernel_size=2, stride=2, bias=False)))
        self.features = nn.Sequential(*layers)
        self.avgpool = nn.AdaptiveAvgPool2d(1)

        last = block_setting[-1]
        last_channels = last.out_channels if last.out_channels is not None else last.input_channels
        self.classifier = nn.Sequential(norm_layer(last_channels), conv_layer(last_channels, num_classes, kernel_size=1, bias=False))
        self.num_classes = num_classes
        self.logit_layer = LogitLayer(logit_temperature=logit_temperature, logit_bias=logit_bias or -math.log(num_classes - 1))

        for m in self.modules():
            if isinstance(m, (nn.Conv2d, nn.Linear)):
                nn.init.trunc_normal_(m.weight, std=0.02)
                if m.bias is not None:
                    nn.init.zeros_(m.bias)

    def _forward_impl(self, x: Tensor) -> Tensor:
        x = self.features(x)
        x = self.classifier(x)          # per position, ahead of the pool
        x = self.avgpool(x)
        x = torch.flatten(x, 1)
        return self.logit_layer(x)

    def forward(self, x: Tensor) -> Tensor:
        engine = getattr(self, "_bcos_engine", None)
        if engine is not None and not torch.is_grad_enabled() and not self.training:
            return engine.forward(x)          # eval + no_grad: the fused plan (bcos_hip/convnext_engine.py)
        return self._forward_impl(x)

    def get_classifier(self) -> nn.Module:
        """the classifier part of the model (it runs before the global pool)"""
        return self.classifier

    def get_feature_extractor(self) -> nn.Module:
        """the feature extractor, without the global pool"""
        return self.features


_STAGES = {
    "convnext_atto": ([(40, 80, 2), (80, 160, 2), (160, 320, 6), (320, None, 2)], 0.1),
    "convnext_tiny": ([(96, 192, 3), (192, 384, 3), (384, 768, 9), (768, None, 3)], 0.1),
    "convnext_small": ([(96, 192, 3), (192, 384, 3), (384, 768, 27), (768, None, 3)], 0.4),
    "convnext_base": ([(128, 256, 3), (256, 512, 3), (512, 1024, 27), (1024, None, 3)], 0.5),
    "convnext_large": ([(192, 384, 3), (384, 768, 3), (768, 1536, 27), (1536, None, 3)], 0.5),
}


def _convnext(arch: str, pretrained: bool, progress: bool, **kwargs: Any) -> BcosConvNeXt:
    stages, sd_default = _STAGES[arch]
    sd_prob = kwargs.pop("stochastic_depth_prob", sd_default)
    if pretrained:
        raise ValueError("pretrained weights are loaded through a state dict (the keys are the reference's), not by this entry point")
    return BcosConvNeXt([CNBlockConfig(*s) for s in stages], stochastic_depth_prob=sd_prob, **kwargs)


def convnext_atto(*, pretrained: bool = False, progress: bool = True, **kwargs: Any) -> BcosConvNeXt:
    return _convnext("convnext_atto", pretrained, progress, **kwargs)


def convnext_tiny(*, pretrained: bool = False, progress: bool = True, **kwargs: Any) -> BcosConvNeXt:
    return _convnext("convnext_tiny", pretrained, progress, **kwargs)


def convnext_small(*, pretrained: bool = False, progress: bool = True, **kwargs: Any) -> BcosConvNeXt:
    return _convnext("convnext_small", pretrained, progress, **kwargs)


def convnext_base(*, pretrained: bool = False, progress: bool = True, **kwargs: Any) -> BcosConvNeXt:
    return _convnext("convnext_base", pretrained, progress, **kwargs)


def convnext_large(*, pretrained: bool = False, progress: bool = True, **kwargs: Any) -> BcosConvNeXt:
    return _convnext("convnext_large", pretrained, progress, **kwargs)
