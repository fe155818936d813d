"""Model zoo entry kept under the reference's module path (models/__init__.py:17-46).  Built natively: the
classifier of the benchmarked path (vgg19_bn, the `else` default of the reference's table), the certification
script's default (resnext29_8_64) and wideresnet28_10; the other architectures of the reference zoo are out of scope
(SURVEY §2, row 4).  DenseNet-BC-100-12 (models/densenet.py) is built natively too and exported here, but the name table below —
which only the reference's training scripts use — does not build it: a checkpoint loads through create_model(path)."""
from .densenet import DenseNet  # noqa: F401
from .resnext import CifarResNeXt  # noqa: F401
from .vgg import VGG, vgg19_bn  # noqa: F401
from .wideresnet import WideResNet  # noqa: F401

available_models = ['vgg19_bn', 'resnext29_8_64', 'wideresnet28_10']


def create_model(model_name, num_classes, in_channels):
    if model_name == 'resnext29_8_64':
        return CifarResNeXt(nlabels=num_classes, in_channels=in_channels)
    if model_name == 'wideresnet28_10':
        return WideResNet(depth=28, widen_factor=10, dropRate=0, num_classes=num_classes, in_channels=in_channels)
    if model_name != 'vgg19_bn':
        raise NotImplementedError('%s is not built natively for MI355X yet (vgg19_bn, resnext29_8_64, wideresnet28_10)' % model_name)
    return vgg19_bn(num_classes=num_classes, in_channels=in_channels)
