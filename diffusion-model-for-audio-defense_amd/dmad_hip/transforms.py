"""The reference's Wave2Spect transforms as HIP-backed callables: the SC09 one (certified_robustness_eval.py:85-87:
torchaudio MelSpectrogram(n_fft=2048, hop_length=512, n_mels=32, norm='slaney', pad_mode='constant',
mel_scale='slaney') followed by AmplitudeToDB(stype='power')) and the keyword spotter's (kws_adaptive_attack_eval.py:74-76:
MelSpectrogram(sample_rate=16000, n_mels=32) with torchaudio's defaults, then the same AmplitudeToDB)."""
import torch

from . import autograd as _ag
from . import engine as _eng


class _EngineTransform(torch.nn.Module):
    """an engine (the shared one by default) and the backend of the gradient branch"""

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


class MelSpectrogramDB(_EngineTransform):
    """[B,1,16000] fp32 CUDA -> [B,1,32,32] dB mel spectrogram (windowed DFT on the fp32 matrix cores,
    |.|^2, slaney filterbank, 10*log10(max(.,1e-10))).

    grad_backend: the gradient branch (x.requires_grad under autograd): 'torch' = the torch restatement (autograd.mel_db), 'hip' = the
    engine's forward and mel VJP (autograd.MelDBHIP), 'auto' (the default) = 'torch'."""

    def forward(self, x):
        if _ag.needs_grad(x):                  # callers that differentiate through the system
            if self.grad_backend == 'hip':
                return _ag.mel_db_hip(self.engine, x)
            return _ag.mel_db(x)
        with torch.no_grad():
            return self.engine.mel_db(x)


Wave2Spect = MelSpectrogramDB


class KWSMelSpectrogramDB(_EngineTransform):
    """The keyword spotter's front-end: [B,1,L] fp32 -> [B,1,32,1 + L // 200] dB mel spectrogram for any L >= 201 (n_fft 400, hop 200,
    reflect padding, htk scale).  On the GPU it is one launch of the engine (kws_mel_db); a CPU input takes the torch
    restatement (autograd.kws_mel_db), like KWSModel's own CPU path.

    grad_backend as for MelSpectrogramDB: 'torch' = autograd.kws_mel_db, 'hip' = the engine's forward and VJP (autograd.KWSMelDBHIP)."""
    _dmad_stage = 'kws_mel_db'

    def forward(self, x):
        if not x.is_cuda:
            return _ag.kws_mel_db(x)
        if _ag.needs_grad(x):
            if self.grad_backend == 'hip':
                return _ag.kws_mel_db_hip(self.engine, x)
            return _ag.kws_mel_db(x)
        with torch.no_grad():
            return self.engine.kws_mel_db(x).unsqueeze(1)
