"""The reference's Wave2Spect transform (certified_robustness_eval.py:85-87:
torchaudio MelSpectrogram(n_fft=2048, hop_length=512, n_mels=32, norm='slaney', pad_mode='constant',
mel_scale='slaney') followed by AmplitudeToDB(stype='power')) as one HIP-backed callable."""
import torch

from . import autograd as _ag
from . import engine as _eng


class MelSpectrogramDB(torch.nn.Module):
    """[B,1,16000] fp32 CUDA -> [B,1,32,32] dB mel spectrogram (windowed DFT on the fp32 matrix cores,
    |.|^2, slaney filterbank, 10*log10(max(.,1e-10))).

    grad_backend: the gradient branch (x.requires_grad under autograd): 'torch' = the torch restatement (autograd.mel_db), 'hip' = the
    engine's forward and mel VJP (autograd.MelDBHIP), 'auto' (the default) = 'torch'."""

    GRAD_BACKENDS = ('auto', 'torch', 'hip')

    def __init__(self, engine=None, grad_backend='auto'):
        super().__init__()
        self._engine = engine
        self.grad_backend = grad_backend

    @property
    def grad_backend(self):
        return self.__dict__.get('_grad_backend', 'auto')

    @grad_backend.setter
    def grad_backend(self, value):
        if value not in self.GRAD_BACKENDS:
            raise ValueError('grad_backend must be one of %s, not %r' % (self.GRAD_BACKENDS, value))
        self.__dict__['_grad_backend'] = value

    @property
    def engine(self):
        if self._engine is None:
            self._engine = _eng.get_engine()
        return self._engine

    def forward(self, x):
        if _ag.needs_grad(x):                  # callers that differentiate through the system
            if self.grad_backend == 'hip':
                return _ag.mel_db_hip(self.engine, x)
            return _ag.mel_db(x)
        with torch.no_grad():
            return self.engine.mel_db(x)


Wave2Spect = MelSpectrogramDB
