"""Attention-CRNN keyword spotter (reference audio_models/RCNN_KWS/model.py:5-114), the classifier of the reference's second task
(kws_adaptive_attack_eval.py): a dB mel spectrogram [B,1,in_size,T] -> depthwise + pointwise Conv1d -> 2-layer bidirectional GRU ->
additive attention over time -> bias-free Linear -> log_softmax, [B,num_classes].  144 k parameters in 24 tensors; class names,
constructor arguments and state-dict keys are the reference's, so its shipped state dicts load as they are (load_checkpoint).
use_engine() puts it on the engine: one fused HIP launch per forward (dmad_kws_logits) and, with grad_backend = 'hip', the engine's
input VJP (dmad_kws_vjp); DESIGN section 22."""
import torch
import torch.nn as nn
import torch.nn.functional as F


def sepconv(in_size, out_size, kernel_size, stride=1, dilation=1, padding=0):
    """depthwise Conv1d over time (kernel_size[1], stride[1]) then a 1-tap Conv1d to out_size (stride[0], in_size // kernel_size[0] groups)"""
    return nn.Sequential(
        nn.Conv1d(in_size, in_size, kernel_size[1], stride=stride[1], dilation=dilation, groups=in_size, padding=padding),
        nn.Conv1d(in_size, out_size, kernel_size=1, stride=stride[0], groups=int(in_size / kernel_size[0])))


class CRNN(nn.Module):
    def __init__(self, in_size, hidden_size, kernel_size, stride, gru_nl):
        super().__init__()
        self.sepconv = sepconv(in_size=in_size, out_size=hidden_size, kernel_size=kernel_size, stride=stride)
        self.gru = nn.GRU(input_size=hidden_size, hidden_size=hidden_size, num_layers=gru_nl, bidirectional=True)

    def forward(self, x, hidden):
        x = self.sepconv(x).permute(2, 0, 1)     # [B, hidden, steps] -> sequence first
        if x.is_cuda and not self.training and torch.is_grad_enabled():
            # MIOpen's fused RNN keeps what its backward needs only in training mode ("RNN backward can only be called in training
            # mode"): an eval-mode gradient, which every attack on this classifier takes, runs torch's own GRU cells instead
            with torch.backends.cudnn.flags(enabled=False):
                return self.gru(x, hidden)
        return self.gru(x, hidden)               # ([steps, B, 2 * hidden], [2 * layers, B, hidden])


class AttnMech(nn.Module):
    def __init__(self, lin_size):
        super().__init__()
        self.Wx_b = nn.Linear(lin_size, lin_size)
        self.Vt = nn.Linear(lin_size, 1, bias=False)

    def forward(self, x):
        return self.Vt(torch.tanh(self.Wx_b(x)))


class ApplyAttn(nn.Module):
    def __init__(self, in_size, num_classes):
        super().__init__()
        self.U = nn.Linear(in_size, num_classes, bias=False)

    def forward(self, e, data):
        a = F.softmax(e, dim=-1).unsqueeze(1)                    # [B, 1, steps]
        c = torch.bmm(a, data.transpose(0, 1)).squeeze()         # the reference's squeeze(): [hidden * dirs] at B = 1
        return F.log_softmax(self.U(c), dim=-1)


class KWSModel(nn.Module):
    # attribute names (CRNN_model, attn_layer, apply_attn) are fixed by the shipped state dicts
    def __init__(self, in_size=40, hidden_size=64, kernel_size=(20, 5), stride=(8, 2), gru_num_layers=2, num_dirs=2, num_classes=4):
        super().__init__()
        self.in_size, self.hidden_size, self.kernel_size, self.stride = in_size, hidden_size, kernel_size, stride
        self.gru_num_layers, self.num_dirs, self.num_classes = gru_num_layers, num_dirs, num_classes
        self.CRNN_model = CRNN(in_size, hidden_size, kernel_size, stride, gru_num_layers)
        self.attn_layer = AttnMech(hidden_size * num_dirs)
        self.apply_attn = ApplyAttn(hidden_size * 2, num_classes)

    GRAD_BACKENDS = ('auto', 'torch', 'hip')

    @property
    def grad_backend(self):
        """Backend of the gradient branch (batch.requires_grad under autograd) once an engine is in use: 'torch' = the module's own
        layers (weight gradients included), 'hip' = the engine's forward and input VJP (dmad_hip.autograd.KWSHIP; input gradient only),
        'auto' (the default) = 'torch'."""
        return self.__dict__.get('_grad_backend', 'auto')

    @grad_backend.setter
    def grad_backend(self, value):
        if value not in self.GRAD_BACKENDS:
            raise ValueError('grad_backend must be one of %s, not %r' % (self.GRAD_BACKENDS, value))
        self.__dict__['_grad_backend'] = value

    def use_engine(self, engine=None):
        """Upload the weights into `engine` as its KWS part (once); None: the shared engine, or an engine of this module's own when the
        shared one already serves a different KWS model.  An explicit engine that holds another KWS model is refused (DmadError).
        Deliberately not called bind_engine, like M5.use_engine: RobustCertificate and build_front bind whatever has that name as the
        32 x 32 spectrogram classifier, and a default KWSModel stays the plain torch module it is."""
        from dmad_hip import engine as _eng
        self.__dict__['engine'] = _eng.bind_kws(self.state_dict(), self.kernel_size, self.stride, engine)
        return self

    def __getstate__(self):
        state = dict(self.__dict__)
        state.pop('engine', None)                 # an engine is a device handle: a copy or a pickle is unbound again
        return state

    def forward(self, batch, hidden=None):
        """batch: dB spectrogram [B, 1, in_size, T] (or [B, in_size, T]) -> log-probabilities [B, num_classes]"""
        x = batch.squeeze(1) if batch.ndim == 4 else batch
        eng = self.__dict__.get('engine')
        if eng is not None and hidden is None and not self.training and x.is_cuda:
            if not (torch.is_grad_enabled() and x.requires_grad):
                return eng.kws_logits(x)
            if self.grad_backend == 'hip':
                from dmad_hip.autograd import kws_hip
                return kws_hip(eng, x)
        if hidden is None:                        # float32 whatever x is, as in the reference: a float64 run passes its own `hidden`
            hidden = torch.zeros(self.gru_num_layers * 2, x.shape[0], self.hidden_size).to(x.device)
        output, hidden = self.CRNN_model(x, hidden)
        e = torch.cat([self.attn_layer(el) for el in output], dim=1)         # [B, steps]
        probs = self.apply_attn(e, output)
        return probs.unsqueeze(0) if probs.ndim == 1 else probs


def is_kws(module) -> bool:
    """True for a KWSModel of this file under any module path it may have been imported by"""
    t = type(module)
    return t.__name__ == 'KWSModel' and t.__module__.split('.')[-1] == 'model' and hasattr(module, 'CRNN_model')


def load_checkpoint(path, map_location='cpu', **kwargs):
    """KWSModel(in_size=32, **kwargs) in eval mode with the state dict at `path`.  The shipped files are plain state dicts saved from
    cuda:0, hence map_location."""
    model = KWSModel(**dict({'in_size': 32}, **kwargs))
    model.load_state_dict(torch.load(path, map_location=map_location))
    return model.eval()
