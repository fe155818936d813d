"""DenseNet for 1x32x32 mel spectrograms (Huang, Liu, van der Maaten & Weinberger, Densely Connected Convolutional Networks,
arXiv:1608.06993; the reference zoo's `densenet_bc_100_12` = DenseNet(depth=100, growthRate=12, compressionRate=2) with the Bottleneck
block) as a HIP-backed module.  Constructor signatures, attribute names and state-dict keys are the reference's (`conv1`,
`dense{1,2,3}.{k}.{bn1,conv1,bn2,conv2}`, `trans{1,2}.{bn1,conv1}`, `bn`, `fc`), so state dicts and pickled checkpoints
(`models.densenet.DenseNet` inside a DataParallel) load unchanged.

A Bottleneck layer: o = relu(bn1(x)), h = relu(bn2(conv1(o))) with 4 * growthRate channels, y = conv2(h) with growthRate channels,
out = cat(x, y).  A Transition: avg_pool2d(conv1(relu(bn1(x))), 2).

The forward runs in libdmad_hip.so (dmad_classify: DESIGN §24).  The gradient branch (x.requires_grad) runs the module's own layers, or
with grad_backend = 'hip' the engine's input VJP (dmad_dn_vjp).  `torch_forward` is those layers on any device."""
import math

import torch
import torch.nn as nn
import torch.nn.functional as F

__all__ = ['DenseNet']


class Bottleneck(nn.Module):

    def __init__(self, inplanes, expansion=4, growthRate=12, dropRate=0):
        super().__init__()
        self.bn1 = nn.BatchNorm2d(inplanes)
        self.conv1 = nn.Conv2d(inplanes, expansion * growthRate, kernel_size=1, bias=False)
        self.bn2 = nn.BatchNorm2d(expansion * growthRate)
        self.conv2 = nn.Conv2d(expansion * growthRate, growthRate, kernel_size=3, padding=1, bias=False)
        self.relu = nn.ReLU(inplace=True)
        self.dropRate = dropRate

    def forward(self, x):
        y = self.conv2(self.relu(self.bn2(self.conv1(self.relu(self.bn1(x))))))
        if self.dropRate > 0:
            y = F.dropout(y, p=self.dropRate, training=self.training)
        return torch.cat((x, y), 1)


class BasicBlock(nn.Module):

    def __init__(self, inplanes, expansion=1, growthRate=12, dropRate=0):
        super().__init__()
        self.bn1 = nn.BatchNorm2d(inplanes)
        self.conv1 = nn.Conv2d(inplanes, growthRate, kernel_size=3, padding=1, bias=False)
        self.relu = nn.ReLU(inplace=True)
        self.dropRate = dropRate

    def forward(self, x):
        y = self.conv1(self.relu(self.bn1(x)))
        if self.dropRate > 0:
            y = F.dropout(y, p=self.dropRate, training=self.training)
        return torch.cat((x, y), 1)


class Transition(nn.Module):

    def __init__(self, inplanes, outplanes):
        super().__init__()
        self.bn1 = nn.BatchNorm2d(inplanes)
        self.conv1 = nn.Conv2d(inplanes, outplanes, kernel_size=1, bias=False)
        self.relu = nn.ReLU(inplace=True)

    def forward(self, x):
        return F.avg_pool2d(self.conv1(self.relu(self.bn1(x))), 2)


class DenseNet(nn.Module):

    def __init__(self, depth=22, block=Bottleneck, dropRate=0, num_classes=10, growthRate=12, compressionRate=2, in_channels=3):
        super().__init__()
        if (depth - 4) % 3 != 0:
            raise ValueError('depth must be 3 n + 4, not %d' % depth)
        n = (depth - 4) // 3 if block is BasicBlock else (depth - 4) // 6
        self.growthRate = growthRate
        self.dropRate = dropRate
        self.inplanes = 2 * growthRate                 # the running width: every helper below advances it
        self.conv1 = nn.Conv2d(in_channels, self.inplanes, kernel_size=3, padding=1, bias=False)
        self.dense1 = self._make_denseblock(block, n)
        self.trans1 = self._make_transition(compressionRate)
        self.dense2 = self._make_denseblock(block, n)
        self.trans2 = self._make_transition(compressionRate)
        self.dense3 = self._make_denseblock(block, n)
        self.bn = nn.BatchNorm2d(self.inplanes)
        self.relu = nn.ReLU(inplace=True)
        self.avgpool = nn.AvgPool2d(8)
        self.fc = nn.Linear(self.inplanes, num_classes)
        for m in self.modules():
            if isinstance(m, nn.Conv2d):
                m.weight.data.normal_(0, math.sqrt(2. / (m.kernel_size[0] * m.kernel_size[1] * m.out_channels)))
            elif isinstance(m, nn.BatchNorm2d):
                m.weight.data.fill_(1); m.bias.data.zero_()

    def _make_denseblock(self, block, blocks):
        layers = []
        for _ in range(int(blocks)):
            layers.append(block(self.inplanes, growthRate=self.growthRate, dropRate=self.dropRate))
            self.inplanes += self.growthRate
        return nn.Sequential(*layers)

    def _make_transition(self, compressionRate):
        inplanes, self.inplanes = self.inplanes, self.inplanes // compressionRate
        return Transition(inplanes, self.inplanes)

    GRAD_BACKENDS = ('auto', 'torch', 'hip')

    @property
    def grad_backend(self):
        """Backend of the gradient branch (x.requires_grad under autograd): 'torch' = the module's own layers (MIOpen, weight gradients
        included), 'hip' = the engine's fp32 tier and DenseNet VJP (dmad_hip.autograd.DNHIP; input gradient only), 'auto' (the default)
        = 'torch'."""
        return self.__dict__.get('_grad_backend', 'auto')

    @grad_backend.setter
    def grad_backend(self, value):
        if value not in self.GRAD_BACKENDS:
            raise ValueError('grad_backend must be one of %s, not %r' % (self.GRAD_BACKENDS, value))
        self.__dict__['_grad_backend'] = value

    # -- HIP engine binding ---------------------------------------------------------------------
    def _is_bc_100_12(self):
        blocks = (self.dense1, self.dense2, self.dense3)
        return (tuple(self.conv1.weight.shape) == (24, 1, 3, 3) and self.growthRate == 12 and self.fc.in_features == 342 and
                all(len(b) == 16 and all(isinstance(layer, Bottleneck) and layer.dropRate == 0 for layer in b) for b in blocks) and
                self.trans1.conv1.out_channels == 108 and self.trans2.conv1.out_channels == 150)

    def bind_engine(self, engine=None):
        """Fold the BatchNorms (eval statistics) and upload the weights into the engine (once).  Only DenseNet-BC-100-12 with one input
        channel and no dropout is built natively; an explicit `engine` that already holds ANOTHER classifier is refused (DmadError)."""
        from dmad_hip import engine as _eng
        if not self._is_bc_100_12():
            raise NotImplementedError('only DenseNet-BC-100-12 (depth 100, growthRate 12, compressionRate 2, Bottleneck) with 1 input channel '
                                      'and dropRate = 0 is built natively for MI355X')
        eng = _eng.bind_classifier(self.state_dict(), 'load_densenet_bc_100_12', engine)
        self.__dict__['engine'] = eng
        return self

    def torch_forward(self, x):
        """the module's own layers (any device; BatchNorm follows the module's mode: eval = its running statistics)"""
        x = self.dense3(self.trans2(self.dense2(self.trans1(self.dense1(self.conv1(x))))))
        x = self.avgpool(self.relu(self.bn(x)))
        return self.fc(x.view(x.size(0), -1))

    def forward(self, x):
        if self.training:
            raise NotImplementedError('the HIP DenseNet is inference-only: call .eval() first')
        if torch.is_grad_enabled() and x.requires_grad and self.grad_backend == 'hip':
            if 'engine' not in self.__dict__:
                self.bind_engine()
            from dmad_hip.autograd import dn_hip
            return dn_hip(self.__dict__['engine'], x)
        if torch.is_grad_enabled() and x.requires_grad:
            if not x.is_cuda:
                raise NotImplementedError('the DenseNet mirror has no CPU path through forward (gradient branch included): torch_forward runs the layers')
            return self.torch_forward(x)
        if 'engine' not in self.__dict__:
            self.bind_engine()
        return self.__dict__['engine'].classify(x)
