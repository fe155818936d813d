"""What the two backends of the baseline waveform defenses share: the host-side filter design (one routine per design) and the
'host' backend's differentiable torch / scipy operators, which run on any device and are the oracle of the GPU tests.

    butter_lowpass / butter_bandpass   scipy.signal.buttord + butter with the reference's arguments (frequency_defense.py:82-86, 122-126),
                                       coefficients rounded to fp32 as the reference's torch.tensor(..., dtype=torch.float) does
    sinc_resample_kernel               torchaudio's published algorithm (functional._get_sinc_resample_kernel: Hann window,
                                       lowpass_filter_width 6, rolloff 0.99), indices in float64, kernel cast to fp32
"""
import functools
import math

import numpy as np
import torch
import torch.nn.functional as F


@functools.lru_cache(maxsize=None)
def butter_lowpass(fs, wp, ws, gpass, gstop):
    from scipy import signal
    wp, ws = 2 * wp / fs, 2 * ws / fs                       # ws = 8000 at fs = 16000 gives ws = 1.0, as in the reference
    N, Wn = signal.buttord(wp, ws, gpass, gstop, analog=False, fs=None)
    b, a = signal.butter(N, Wn, btype='low', analog=False, output='ba')
    return np.asarray(b, dtype=np.float32), np.asarray(a, dtype=np.float32), int(N), Wn


@functools.lru_cache(maxsize=None)
def butter_bandpass(fs, wp, ws, gpass, gstop):
    from scipy import signal
    wp, ws = [2 * w / fs for w in wp], [2 * w / fs for w in ws]
    N, Wn = signal.buttord(wp, ws, gpass, gstop, analog=False, fs=None)
    b, a = signal.butter(N, Wn, btype='bandpass', analog=False, output='ba', fs=None)
    return np.asarray(b, dtype=np.float32), np.asarray(a, dtype=np.float32), int(N), Wn


@functools.lru_cache(maxsize=None)
def sinc_resample_kernel(orig_freq: int, new_freq: int, lowpass_filter_width: int = 6, rolloff: float = 0.99):
    """-> (kernel fp32 [new][2 * width + orig], width, orig, new) with orig / new reduced by their gcd.  A clip of L samples is padded
    with (width, width + orig) zeros, convolved with stride orig, the `new` phases interleaved and cut to ceil(new * L / orig)."""
    g = math.gcd(int(orig_freq), int(new_freq))
    orig, new = int(orig_freq) // g, int(new_freq) // g
    base_freq = min(orig, new) * rolloff
    width = math.ceil(lowpass_filter_width * orig / base_freq)
    idx = np.arange(-width, width + orig, dtype=np.float64)[None, :] / orig
    t = np.arange(0, -new, -1, dtype=np.float64)[:, None] / new + idx
    t = np.clip(t * base_freq, -lowpass_filter_width, lowpass_filter_width)
    window = np.cos(t * math.pi / lowpass_filter_width / 2) ** 2
    t = t * math.pi
    scale = base_freq / orig
    safe = np.where(t == 0, 1.0, t)
    kernel = np.where(t == 0, 1.0, np.sin(safe) / safe) * window * scale
    kernel = np.ascontiguousarray(kernel, dtype=np.float32)
    kernel.setflags(write=False)
    return kernel, int(width), orig, new


def resample_length(L: int, orig: int, new: int) -> int:
    return int(math.ceil(new * L / orig))


# ------------------------------------------------------------------------------------------------------------ 'host' operators
def host_mean(x: torch.Tensor, window: int) -> torch.Tensor:
    """[B,T] -> [B,T]: F.conv1d with the fp32 1 / w kernel, zero padding (time_defense.py:122-124)."""
    weight = torch.tensor(np.ones(window) / window, dtype=torch.float, device=x.device).to(x.dtype).view(1, 1, -1)
    return F.conv1d(x.unsqueeze(1), weight, padding=(window - 1) // 2).squeeze(1)


def host_median(x: torch.Tensor, window: int) -> torch.Tensor:
    """[B,T] -> [B,T]: zero padding, unfold, torch.median (time_defense.py:148-156)."""
    p = (window - 1) // 2
    roll = F.pad(x, (p, p), mode='constant', value=0.).unfold(-1, window, 1)
    return torch.median(roll, -1)[0]


def host_resample(x: torch.Tensor, kernel: np.ndarray, width: int, orig: int, L_out: int) -> torch.Tensor:
    """[B,L] -> [B,L_out]: torchaudio's _apply_sinc_resample_kernel."""
    k = torch.from_numpy(np.array(kernel)).to(device=x.device, dtype=x.dtype).unsqueeze(1)
    y = F.conv1d(F.pad(x, (width, width + orig)).unsqueeze(1), k, stride=orig)
    return y.transpose(1, 2).reshape(x.shape[0], -1)[..., :L_out]


class HostIIR(torch.autograd.Function):
    """y = lfilter(b, a, x) along the last axis: scipy.signal.lfilter in float64 on the CPU, cast back to x's dtype and device.  The
    backward is the flipped filter, g_x = flip(lfilter(b, a, flip(g_y)))."""

    @staticmethod
    def _run(b, a, x):
        from scipy import signal
        y = signal.lfilter(np.asarray(b, dtype=np.float64), np.asarray(a, dtype=np.float64), x.detach().cpu().double().numpy(), axis=-1)
        return torch.from_numpy(np.ascontiguousarray(y)).to(device=x.device, dtype=x.dtype)

    @staticmethod
    def forward(ctx, x, b, a):
        ctx.b, ctx.a = b, a
        return HostIIR._run(b, a, x)

    @staticmethod
    def backward(ctx, g_y):
        return HostIIR._run(ctx.b, ctx.a, g_y.flip(-1)).flip(-1), None, None


def host_iir(x: torch.Tensor, b, a, lo: float, hi: float) -> torch.Tensor:
    return HostIIR.apply(x, b, a).clamp(lo, hi)


# ------------------------------------------------------------------------------------------------------------ shapes and backends
def as_rows(audio: torch.Tensor):
    """The reference's shape handling: (T,), (B,T) or (B,1,T) -> ([B,T], original shape)."""
    assert torch.is_tensor(audio) == True   # noqa: E712
    ori_shape = audio.shape
    if len(audio.shape) == 1:
        audio = audio.unsqueeze(0)
    elif len(audio.shape) == 2:
        pass
    elif len(audio.shape) == 3:
        audio = audio.squeeze(1)
    else:
        raise NotImplementedError('Audio Shape Error')
    return audio, ori_shape


def pick_backend(x: torch.Tensor, backend, engine):
    """-> ('hip', engine) or ('host', None).  backend None: 'hip' for CUDA input when an engine is at hand (the one passed, or the
    process-wide engine if it exists already), 'host' otherwise."""
    if backend not in (None, 'hip', 'host'):
        raise ValueError("backend must be 'hip' or 'host', not %r" % (backend,))
    if backend == 'host':
        return 'host', None
    if backend is None:
        if not x.is_cuda:
            return 'host', None
        if engine is None:
            from dmad_hip import engine as E
            engine = next((e for (dev, _), e in E._ENGINES.items() if dev == x.device.index), None)
        return ('hip', engine) if engine is not None else ('host', None)
    if engine is None:
        from dmad_hip import engine as E
        engine = E.get_engine()
    return 'hip', engine
