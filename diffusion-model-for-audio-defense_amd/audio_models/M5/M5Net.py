"""M5 raw-waveform classifier (reference audio_models/M5/M5Net.py:4-38), needed so that the bundled
whole-module M5 pickles (`M5Net.M5`) can be unpickled by create_model().  27.8 k parameters: it is
not on the MFMA-bound part of the path and, as created, runs as ordinary torch ops on whatever device it is on
(SURVEY section 2, row 5).  use_engine() puts it on the engine: one fused HIP launch per forward (dmad_m5_logits) and, with
grad_backend = 'hip', the engine's input VJP (dmad_m5_vjp); DESIGN section 19."""
import torch
import torch.nn as nn
import torch.nn.functional as F


class M5(nn.Module):
    # attribute names (conv1..4, bn1..4, pool1..4, fc1) are fixed by the pickled checkpoints
    def __init__(self, n_input=1, first_kernel_size=80, n_output=35, stride=16, n_channel=32):
        super().__init__()
        widths = [(n_input, n_channel, first_kernel_size, stride), (n_channel, n_channel, 3, 1),
                  (n_channel, 2 * n_channel, 3, 1), (2 * n_channel, 2 * n_channel, 3, 1)]
        for i, (cin, cout, k, s) in enumerate(widths, start=1):
            setattr(self, 'conv%d' % i, nn.Conv1d(cin, cout, kernel_size=k, stride=s))
            setattr(self, 'bn%d' % i, nn.BatchNorm1d(cout))
            setattr(self, 'pool%d' % i, nn.MaxPool1d(4))
        self.fc1 = nn.Linear(2 * n_channel, n_output)

    GRAD_BACKENDS = ('auto', 'torch', 'hip')

    @property
    def grad_backend(self):
        """Backend of the gradient branch (x.requires_grad under autograd) once an engine is in use: 'torch' = the module's own layers
        (weight gradients included), 'hip' = the engine's forward and input VJP (dmad_hip.autograd.M5HIP; input gradient only),
        'auto' (the default) = 'torch'."""
        return self.__dict__.get('_grad_backend', 'auto')

    @grad_backend.setter
    def grad_backend(self, value):
        if value not in self.GRAD_BACKENDS:
            raise ValueError('grad_backend must be one of %s, not %r' % (self.GRAD_BACKENDS, value))
        self.__dict__['_grad_backend'] = value

    def use_engine(self, engine=None):
        """Fold BatchNorm (eval statistics) and upload the weights into `engine` as its M5 part (once); None: the shared engine, or an
        engine of this module's own when the shared one already serves a different M5.  An explicit engine that holds another M5 is
        refused (DmadError).  Deliberately not called bind_engine: RobustCertificate and build_front bind whatever has that name, and a
        default M5 stays the plain torch module it is."""
        from dmad_hip import engine as _eng
        self.__dict__['engine'] = _eng.bind_m5(self.state_dict(), self.conv1.stride[0], engine)
        return self

    def __getstate__(self):
        state = dict(self.__dict__)
        state.pop('engine', None)                 # an engine is a device handle: a copy or a pickle is unbound again
        return state

    def forward(self, x):
        eng = self.__dict__.get('engine')
        if eng is not None and not self.training and x.is_cuda:
            if not (torch.is_grad_enabled() and x.requires_grad):
                return eng.m5_logits(x)
            if self.grad_backend == 'hip':
                from dmad_hip.autograd import m5_hip
                return m5_hip(eng, x)
        for i in (1, 2, 3, 4):
            x = getattr(self, 'conv%d' % i)(x)
            x = getattr(self, 'pool%d' % i)(F.relu(getattr(self, 'bn%d' % i)(x)))
        x = F.avg_pool1d(x, x.shape[-1]).flatten(1)
        return F.log_softmax(self.fc1(x), dim=1)


def is_m5(module) -> bool:
    """True for an M5 of this file under either of its module paths: `M5Net` (the path inside the reference's pickled checkpoints, which
    create_model() makes importable) and `audio_models.M5.M5Net` are two class objects."""
    t = type(module)
    return t.__name__ == 'M5' and t.__module__.split('.')[-1] == 'M5Net'
