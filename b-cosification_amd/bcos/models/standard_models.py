"""ResNetBcos / DenseNetBcos: torchvision-topology networks whose classifier runs BEFORE global average pooling, so that
the B-cosified `fc` / `classifier` (a 1x1 BcosifyConv2d) sees spatial features (reference bcos/models/standard_models.py:36-63)."""
import torch.nn.functional as F

try:  # the reference subclasses torchvision's class; use it when available so user code sees the same type
    from torchvision.models import ResNet
    from torchvision.models.resnet import BasicBlock, Bottleneck
except Exception:  # torchvision absent (MI355X image): restated topology with identical names
    from ._tv_resnet import BasicBlock, Bottleneck, ResNet
try:
    from torchvision.models import DenseNet
except Exception:
    from ._tv_densenet import DenseNet

__all__ = ["ResNetBcos", "MyResNet", "DenseNetBcos", "MyDenseNet", "BasicBlock", "Bottleneck"]


class MyResNet(ResNet):
    """Unmodified ordering (pool, flatten, fc): the non-B-cos baseline of the reference (:7-24)."""


class ResNetBcos(ResNet):
    def _forward_impl(self, x):
        x = self.maxpool(self.relu(self.bn1(self.conv1(x))))
        x = self.layer4(self.layer3(self.layer2(self.layer1(x))))
        x = self.fc(x)               # 1x1 B-cos conv on [N,C,h,w]
        return self.avgpool(x).flatten(1)


class MyDenseNet(DenseNet):
    """Unmodified ordering (relu, pool, flatten, classifier): the non-B-cos baseline of the reference (:25-32)."""


class DenseNetBcos(DenseNet):
    def forward(self, x):
        out = F.relu(self.features(x), inplace=True)      # the ReLU behind norm5 is functional (reference :58-59)
        out = self.classifier(out)                        # 1x1 B-cos conv on [N,C,h,w]
        return F.adaptive_avg_pool2d(out, (1, 1)).flatten(1)
