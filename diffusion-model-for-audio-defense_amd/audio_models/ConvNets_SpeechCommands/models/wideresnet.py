"""WideResNet for 1x32x32 mel spectrograms (Zagoruyko & Komodakis, Wide Residual Networks, arXiv:1605.07146; the reference zoo's
`wideresnet28_10` = WideResNet(depth=28, widen_factor=10, dropRate=0)) as a HIP-backed module.  Constructor signatures, attribute names
and state-dict keys are the reference's (`conv1`, `block{1,2,3}.layer.{k}.{bn1,conv1,bn2,conv2,convShortcut}`, `bn1`, `fc`; `convShortcut`
is None where in == out), so state dicts and pickled checkpoints (`models.wideresnet.WideResNet` inside a DataParallel) load unchanged.

A block is pre-activation: o = relu(bn1(x)), h = relu(bn2(conv1(o))), y = shortcut + conv2(h); conv1 carries the stride.  Where the widths
agree the shortcut is the raw x; in the first block of every stage it is convShortcut(o), the 1x1 conv of the ACTIVATED input.

The forward runs in libdmad_hip.so (dmad_classify: DESIGN §21).  The gradient branch (x.requires_grad) runs the module's own layers, or
with grad_backend = 'hip' the engine's input VJP (dmad_wrn_vjp).  `torch_forward` is those layers on any device."""
import math

import torch
import torch.nn as nn
import torch.nn.functional as F

__all__ = ['WideResNet']


class BasicBlock(nn.Module):

    def __init__(self, in_planes, out_planes, stride, dropRate=0.0):
        super().__init__()
        self.bn1 = nn.BatchNorm2d(in_planes)
        self.relu1 = nn.ReLU(inplace=True)
        self.conv1 = nn.Conv2d(in_planes, out_planes, kernel_size=3, stride=stride, padding=1, bias=False)
        self.bn2 = nn.BatchNorm2d(out_planes)
        self.relu2 = nn.ReLU(inplace=True)
        self.conv2 = nn.Conv2d(out_planes, out_planes, kernel_size=3, stride=1, padding=1, bias=False)
        self.droprate = dropRate
        self.equalInOut = in_planes == out_planes
        self.convShortcut = None if self.equalInOut else nn.Conv2d(in_planes, out_planes, kernel_size=1, stride=stride, padding=0, bias=False)

    def forward(self, x):
        o = self.relu1(self.bn1(x))
        h = self.relu2(self.bn2(self.conv1(o)))
        if self.droprate > 0:
            h = F.dropout(h, p=self.droprate, training=self.training)
        return (x if self.equalInOut else self.convShortcut(o)) + self.conv2(h)


class NetworkBlock(nn.Module):

    def __init__(self, nb_layers, in_planes, out_planes, block, stride, dropRate=0.0):
        super().__init__()
        self.layer = self._make_layer(block, in_planes, out_planes, nb_layers, stride, dropRate)

    def _make_layer(self, block, in_planes, out_planes, nb_layers, stride, dropRate):
        return nn.Sequential(*[block(in_planes if i == 0 else out_planes, out_planes, stride if i == 0 else 1, dropRate)
                               for i in range(int(nb_layers))])

    def forward(self, x):
        return self.layer(x)


class WideResNet(nn.Module):

    def __init__(self, depth, num_classes, in_channels=3, widen_factor=1, dropRate=0.0):
        super().__init__()
        widths = [16, 16 * widen_factor, 32 * widen_factor, 64 * widen_factor]
        if (depth - 4) % 6 != 0:
            raise ValueError('depth must be 6 n + 4, not %d' % depth)
        n = (depth - 4) // 6
        self.conv1 = nn.Conv2d(in_channels, widths[0], kernel_size=3, stride=1, padding=1, bias=False)
        self.block1 = NetworkBlock(n, widths[0], widths[1], BasicBlock, 1, dropRate)
        self.block2 = NetworkBlock(n, widths[1], widths[2], BasicBlock, 2, dropRate)
        self.block3 = NetworkBlock(n, widths[2], widths[3], BasicBlock, 2, dropRate)
        self.bn1 = nn.BatchNorm2d(widths[3])
        self.relu = nn.ReLU(inplace=True)
        self.fc = nn.Linear(widths[3], num_classes)
        self.nChannels = widths[3]
        for m in self.modules():
            if isinstance(m, nn.Conv2d):
                m.weight.data.normal_(0, math.sqrt(2. / (m.kernel_size[0] * m.kernel_size[1] * m.out_channels)))
            elif isinstance(m, nn.BatchNorm2d):
                m.weight.data.fill_(1); m.bias.data.zero_()
            elif isinstance(m, nn.Linear):
                m.bias.data.zero_()

    GRAD_BACKENDS = ('auto', 'torch', 'hip')

    @property
    def grad_backend(self):
        """Backend of the gradient branch (x.requires_grad under autograd): 'torch' = the module's own layers (MIOpen, weight gradients
        included), 'hip' = the engine's fp32 tier and WideResNet VJP (dmad_hip.autograd.WRNHIP; input gradient only), 'auto' (the
        default) = 'torch'."""
        return self.__dict__.get('_grad_backend', 'auto')

    @grad_backend.setter
    def grad_backend(self, value):
        if value not in self.GRAD_BACKENDS:
            raise ValueError('grad_backend must be one of %s, not %r' % (self.GRAD_BACKENDS, value))
        self.__dict__['_grad_backend'] = value

    # -- HIP engine binding ---------------------------------------------------------------------
    def _is_28_10(self):
        return (tuple(self.conv1.weight.shape) == (16, 1, 3, 3) and self.nChannels == 640 and
                all(len(b.layer) == 4 for b in (self.block1, self.block2, self.block3)) and
                all(blk.droprate == 0 for b in (self.block1, self.block2, self.block3) for blk in b.layer))

    def bind_engine(self, engine=None):
        """Fold the BatchNorms (eval statistics) and upload the weights into the engine (once).  Only WideResNet-28-10 with one input
        channel and no dropout is built natively; an explicit `engine` that already holds ANOTHER classifier is refused (DmadError)."""
        from dmad_hip import engine as _eng
        if not self._is_28_10():
            raise NotImplementedError('only WideResNet-28-10 with 1 input channel and dropRate = 0 is built natively for MI355X')
        eng = _eng.bind_classifier(self.state_dict(), 'load_wideresnet28_10', engine)
        self.__dict__['engine'] = eng
        return self

    def torch_forward(self, x):
        """the module's own layers (any device; BatchNorm follows the module's mode: eval = its running statistics)"""
        out = self.block3(self.block2(self.block1(self.conv1(x))))
        out = F.avg_pool2d(self.relu(self.bn1(out)), 8)
        return self.fc(out.view(-1, self.nChannels))

    def forward(self, x):
        if self.training:
            raise NotImplementedError('the HIP WideResNet is inference-only: call .eval() first')
        if torch.is_grad_enabled() and x.requires_grad and self.grad_backend == 'hip':
            if 'engine' not in self.__dict__:
                self.bind_engine()
            from dmad_hip.autograd import wrn_hip
            return wrn_hip(self.__dict__['engine'], x)
        if torch.is_grad_enabled() and x.requires_grad:
            if not x.is_cuda:
                raise NotImplementedError('the WideResNet mirror has no CPU path through forward (gradient branch included): torch_forward runs the layers')
            return self.torch_forward(x)
        if 'engine' not in self.__dict__:
            self.bind_engine()
        return self.__dict__['engine'].classify(x)
