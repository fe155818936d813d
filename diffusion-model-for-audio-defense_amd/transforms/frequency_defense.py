"""Frequency-domain baseline defenses of the attack drivers, at the reference's module path (transforms/frequency_defense.py:7-141):
FreqDomainDefense with DS (down-sampling and back), LPF and BPF (Butterworth low-pass / band-pass, then clamp).  Signatures, defaults,
accepted shapes, _get_name() strings and the NotImplementedError for an unknown type are the reference's, and so are its quirks: LPF and
BPF choose the clamp range from `0.9 * max <= 1 and 0.9 * min >= -1` over the whole batch, and LPF's ws = 8000 at fs = 16000 is ws = 1.0.

The reference resamples with torchaudio and filters with torch_lfilter on the CPU, one clip at a time; neither library is needed here.
backend = 'hip' runs the engine's kernels (dmad_wave_resample, dmad_wave_iir and their VJPs), 'host' runs F.conv1d with the same sinc
kernel and scipy.signal.lfilter in float64 on the CPU.  Both take their coefficients from the one design routine in _wave_design.
Default: 'hip' for CUDA input when an engine is at hand, 'host' otherwise."""
from . import _wave_design as wd


class FreqDomainDefense():

    def __init__(self, defense_type: str, *args, backend=None, engine=None) -> None:
        self.defense_type = defense_type
        self.backend, self.engine = backend, engine

    def __call__(self, x, *args):
        kw = dict(backend=self.backend, engine=self.engine)
        if self.defense_type == 'DS':
            output = DS(x, *args, **kw)
        elif self.defense_type == 'LPF':
            output = LPF(x, *args, **kw)
        elif self.defense_type == 'BPF':
            output = BPF(x, *args, **kw)
        else:
            raise NotImplementedError(f'Unknown defense type: {self.defense_type}!')
        return output

    def _get_name(self, *args):
        if self.defense_type == 'DS':
            name = 'Down_Sampling'
        elif self.defense_type == 'LPF':
            name = 'Low_Pass_Filter'
        elif self.defense_type == 'BPF':
            name = 'Band_Pass_Filter'
        else:
            raise NotImplementedError(f'Unknown defense type: {self.defense_type}!')
        return name

    def engine_defense(self, x):
        """The defense at its defaults as Engine.defense_query_logits takes it (AcousticSystem.query's one-call path); x decides the
        clamp range of LPF / BPF."""
        if self.defense_type == 'DS':
            L = x.shape[-1]
            (dk, dw, do, dn), (uk, uw, uo, un) = wd.sinc_resample_kernel(16000, 8000), wd.sinc_resample_kernel(8000, 16000)
            return dict(kind='DS', down=(dk, do, dw, wd.resample_length(L, do, dn)), up=(uk, uo, uw))
        if self.defense_type == 'LPF':
            b, a = wd.butter_lowpass(16000, 4000, 8000, 3, 40)[:2]
        elif self.defense_type == 'BPF':
            b, a = wd.butter_bandpass(16000, (300, 4000), (50, 8000), 3, 40)[:2]
        else:
            raise NotImplementedError(f'Unknown defense type: {self.defense_type}!')
        lo, hi = _clip_range(x, 16)
        return dict(kind='IIR', b=b, a=a, lo=lo, hi=hi)


def _clip_range(x, bits):
    if 0.9 * x.max() <= 1 and 0.9 * x.min() >= -1:
        return -1, 1
    return -2 ** (bits - 1), 2 ** (bits - 1) - 1


def DS(audio, param=0.5, fs=16000, same_size=True, *, backend=None, engine=None):
    rows, ori_shape = wd.as_rows(audio)
    L = rows.shape[1]
    new_freq = int(fs * param)
    (dk, dw, do, dn), (uk, uw, uo, un) = wd.sinc_resample_kernel(fs, new_freq), wd.sinc_resample_kernel(new_freq, fs)
    L_mid = wd.resample_length(L, do, dn)
    L_up = wd.resample_length(L_mid, uo, un)
    which, eng = wd.pick_backend(rows, backend, engine)
    if which == 'hip':
        from dmad_hip.autograd import WaveResampleHIP
        down = WaveResampleHIP.apply(rows.contiguous().float(), eng, dk, do, dw, L_mid)
        new_audio = WaveResampleHIP.apply(down, eng, uk, uo, uw, L_up).to(rows.dtype)
    else:
        new_audio = wd.host_resample(wd.host_resample(rows, dk, dw, do, L_mid), uk, uw, uo, L_up)
    if same_size:  # sometimes the returned audio may have longer size (usually 1 point)
        return new_audio[..., :L].reshape(ori_shape)
    return new_audio.reshape(ori_shape[:-1] + new_audio.shape[-1:])


def _iir(new, b, a, bits, backend, engine):
    rows, ori_shape = wd.as_rows(new)
    clip_min, clip_max = _clip_range(rows, bits)
    which, eng = wd.pick_backend(rows, backend, engine)
    if which == 'hip':
        from dmad_hip.autograd import WaveIIRHIP
        out = WaveIIRHIP.apply(rows.contiguous().float(), eng, b, a, clip_min, clip_max).to(rows.dtype)
    else:
        out = wd.host_iir(rows, b, a, clip_min, clip_max)
    return out.reshape(ori_shape)


def LPF(new, fs=16000, wp=4000, param=8000, gpass=3, gstop=40, same_size=True, bits=16, *, backend=None, engine=None):
    b, a = wd.butter_lowpass(fs, wp, param, gpass, gstop)[:2]
    return _iir(new, b, a, bits, backend, engine)


def BPF(new, fs=16000, wp=[300, 4000], param=[50, 8000], gpass=3, gstop=40, same_size=True, bits=16, *, backend=None, engine=None):
    b, a = wd.butter_bandpass(fs, tuple(wp), tuple(param), gpass, gstop)[:2]
    return _iir(new, b, a, bits, backend, engine)
