"""The differentiation branch of the host mirrors ("Autograd").

The HIP engine is inference-only.  The reference's white-box attack drivers differentiate THROUGH the system
(`AcousticSystem.forward` with `x.requires_grad`, adaptive_attack_eval.py:176,262; kws_adaptive_attack_eval.py:111 builds the
DDPM `DiffWave` as defender), so the survey's boundary asks the mirrors to take a torch restatement on exactly that branch:
`torch.is_grad_enabled() and x.requires_grad`.  This module holds those restatements — plain differentiable torch ops on the
caller's CUDA tensors, fed with the same folded weights the engine packs:

    wavenet_eps   WaveNet_Speech_Commands.forward   DiffWave_Unconditional/WaveNet.py:75-97,120-135,164-172; util.py:68-93
    mel_db        MelSpectrogram + AmplitudeToDB    certified_robustness_eval.py:85-87 (torchaudio 0.11 semantics)
    kws_mel_db    MelSpectrogram + AmplitudeToDB    kws_adaptive_attack_eval.py:74-76 (n_fft 400, hop 200, reflect padding, htk scale; any L, any device)

(the classifiers' own nn layers are their restatement: models/vgg.py:48-52, models/resnext.py:47-62,133-142).
Scope: gradients only.  Nothing here runs when no gradient is requested — inference calls go to libdmad_hip.so and fail loudly
without it — tensors must live on the GPU like everywhere else in this package, nothing here is timed by bench.py, and nothing
here imports `oracle/` (test infrastructure).  tests/test_gpu_parity.py::test_autograd_branch checks the forward values of this
branch against the HIP fp32 path and its gradients against finite differences taken WITH the HIP fp32 path.

WaveNetEpsHIP is the native alternative for the eps-network (WaveNetHIP(..., grad_backend='hip')): its forward is the engine's
exact-fp32 path and its backward the engine's vector-Jacobian product (dmad_wavenet_eps_vjp), which saves the residual streams
only — no torch activations are kept between forward and backward.

UNetEpsHIP does the same for the Improved-Diffusion UNet of the spectrogram-domain purifier (UNetModel(..., grad_backend='hip')): its
forward is the engine's exact-fp32 UNet tier and its backward the engine's UNet VJP (dmad_unet_eps_vjp), which re-runs the forward
with its tape stored on the device.  There is no torch restatement of the UNet in this package.

ResNeXtHIP and MelDBHIP are the native alternatives for the last two stages of every attack gradient (CifarResNeXt.grad_backend =
'hip', MelSpectrogramDB(..., grad_backend='hip')): the classifier's forward is the engine's fp32 ResNeXt29 tier and its backward the
engine's ResNeXt29 VJP (dmad_classify_vjp, tape re-written on the device); the mel front-end's backward recomputes the forward and
walks dB, filterbank, |.|^2, DFT and overlap-add in reverse (dmad_mel_db_vjp).  Neither computes weight gradients.

KWSMelDBHIP and KWSWaveHIP are the native alternatives for the keyword spotter's front-end and for the front-end with KWSModel behind it
(KWSMelSpectrogramDB(..., grad_backend='hip'); AcousticSystem.forward of a KWSModel behind its own front-end): dmad_kws_mel_db_vjp, and
dmad_kws_wave_vjp, which computes only the spectrogram frames the model reads.
"""
import math

import numpy as np
import torch
import torch.nn.functional as F

from ._lib import DmadError


def needs_grad(x) -> bool:
    return isinstance(x, torch.Tensor) and torch.is_grad_enabled() and x.requires_grad


def _require_cuda(x):
    if not x.is_cuda:
        raise DmadError('input must live on the GPU (this package has no CPU path, the differentiation branch included)')


def _first_order_only(name: str, torch_hint: bool = True):
    """the refusal every backward below starts with; torch_hint: a torch restatement exists to fall back to"""
    if torch.is_grad_enabled():
        raise DmadError('the HIP %s VJP is first-order only: create_graph=True (double backward) is not supported' % name
                        + ("; use grad_backend='torch' for higher derivatives" if torch_hint else ''))


class FoldedWaveNet:
    """Folded fp32 WaveNet weights (dmad_hip.engine.fold_wavenet_state_dict) as device tensors, created on first use."""

    def __init__(self, folded: dict, num_res_layers: int, dilation_cycle: int):
        self.host, self.NL, self.cycle = folded, int(num_res_layers), int(dilation_cycle)
        self._dev = {}

    def on(self, device):
        key = str(device)
        if key not in self._dev:
            w = {k: torch.from_numpy(np.ascontiguousarray(v)).to(device) for k, v in self.host.items()}
            for n in range(self.NL):                        # conv1d weight shapes: [out, in, k]
                w['res.%d.w' % n] = w['res.%d.w' % n].reshape(256, 256, 1)
                w['skip.%d.w' % n] = w['skip.%d.w' % n].reshape(256, 256, 1)
            w['init.w'] = w['init.w'].reshape(256, 1, 1)
            w['f0.w'] = w['f0.w'].reshape(256, 256, 1)
            w['f2.w'] = w['f2.w'].reshape(1, 256, 1)
            self._dev[key] = w
        return self._dev[key]


def wavenet_eps(fw: FoldedWaveNet, audio: torch.Tensor, t: int) -> torch.Tensor:
    """eps = WaveNet((audio [B,1,L], t * ones)), differentiable in `audio`."""
    _require_cuda(audio)
    w = fw.on(audio.device)
    B = audio.shape[0]
    x = torch.relu(F.conv1d(audio, w['init.w'], w['init.b']))
    # calc_diffusion_step_embedding (util.py:84-91): cat(sin, cos)(t * exp(-j ln(1e4) / 63)), j < 64
    half = w['fc_t1.w'].shape[1] // 2
    freq = torch.exp(torch.arange(half, device=audio.device) * -(math.log(10000.0) / (half - 1))).float()
    arg = float(t) * freq
    emb = torch.cat([torch.sin(arg), torch.cos(arg)]).unsqueeze(0).expand(B, -1)
    emb = F.silu(F.linear(emb, w['fc_t1.w'], w['fc_t1.b']))
    emb = F.silu(F.linear(emb, w['fc_t2.w'], w['fc_t2.b']))
    skip = 0
    for n in range(fw.NL):
        d = 2 ** (n % fw.cycle)
        h = x + F.linear(emb, w['fc_t.%d.w' % n], w['fc_t.%d.b' % n]).view(B, -1, 1)       # the reference's in-place alias
        H = F.conv1d(h, w['dil.%d.w' % n], w['dil.%d.b' % n], dilation=d, padding=d)
        g = torch.tanh(H[:, :256]) * torch.sigmoid(H[:, 256:])
        x = (h + F.conv1d(g, w['res.%d.w' % n], w['res.%d.b' % n])) * math.sqrt(0.5)
        skip = skip + F.conv1d(g, w['skip.%d.w' % n], w['skip.%d.b' % n])
    y = torch.relu(F.conv1d(skip * math.sqrt(1.0 / fw.NL), w['f0.w'], w['f0.b']))
    return F.conv1d(y, w['f2.w'], w['f2.b'])


_MEL_CACHE = {}


def _mel_constants(device):
    key = str(device)
    if key not in _MEL_CACHE:
        def hz2mel(f):
            return np.where(f >= 1000.0, 15.0 + np.log(np.maximum(f, 1e-30) / 1000.0) / (np.log(6.4) / 27.0), f / (200.0 / 3))

        def mel2hz(m):
            return np.where(m >= 15.0, 1000.0 * np.exp((np.log(6.4) / 27.0) * (m - 15.0)), (200.0 / 3) * m)
        pts = mel2hz(np.linspace(hz2mel(np.float64(0.0)), hz2mel(np.float64(8000.0)), 34))
        freqs = np.linspace(0.0, 8000.0, 1025)
        down = (freqs[None, :] - pts[:-2, None]) / (pts[1:-1, None] - pts[:-2, None])
        up = (pts[2:, None] - freqs[None, :]) / (pts[2:, None] - pts[1:-1, None])
        fb = np.maximum(0.0, np.minimum(down, up)) * (2.0 / (pts[2:] - pts[:-2]))[:, None]           # slaney norm, [32][1025]
        _MEL_CACHE[key] = (torch.hann_window(2048, periodic=True, device=device), torch.from_numpy(fb).float().to(device))
    return _MEL_CACHE[key]


def mel_db(x: torch.Tensor) -> torch.Tensor:
    """[B,1,16000] -> [B,1,32,32] dB mel spectrogram, differentiable in x."""
    _require_cuda(x)
    win, fb = _mel_constants(x.device)
    spec = torch.stft(x[:, 0], n_fft=2048, hop_length=512, win_length=2048, window=win, center=True, pad_mode='constant',
                      normalized=False, onesided=True, return_complex=True)
    power = spec.real ** 2 + spec.imag ** 2                                        # [B, 1025, 32]
    mel = torch.matmul(fb, power)                                                  # [B, 32, 32]
    return (10.0 * torch.log10(torch.clamp(mel, min=1e-10))).unsqueeze(1)


class WaveNetEpsHIP(torch.autograd.Function):
    """eps = WaveNet((audio [B,1,L], t * ones)) on the engine's exact-fp32 path, differentiable in `audio` through the engine's VJP.
    Saves only the input; the backward re-runs the forward with its residual streams saved (dmad_wavenet_eps_vjp).  The VJP
    workspace is reserved on first use.  First-order only: create_graph=True raises."""

    @staticmethod
    def forward(ctx, audio, engine, t):
        from . import engine as _eng
        _require_cuda(audio)
        if engine.precision == _eng.FP32:
            eps = engine.wavenet_eps(audio, t)
        elif engine.precision == _eng.EXACT:
            eps = engine.wavenet_eps_path(audio, t, _eng.WAVE_FP32)
        else:
            raise DmadError('the HIP VJP runs on the exact-fp32 path: a BF16 engine holds no fp32 weights (use an FP32 or EXACT engine)')
        ctx.engine, ctx.t = engine, int(t)
        ctx.save_for_backward(audio)
        return eps.view(audio.shape)

    @staticmethod
    def backward(ctx, g_eps):
        _first_order_only('WaveNet')
        audio, = ctx.saved_tensors
        eng, B = ctx.engine, audio.shape[0]
        if eng.vjp_batch < B:
            eng.reserve_vjp(B)
        g_x = eng.wavenet_eps_vjp(audio, ctx.t, g_eps.reshape(audio.shape).contiguous())
        return g_x.view(audio.shape).to(audio.dtype), None, None


def wavenet_eps_hip(engine, audio: torch.Tensor, t: int) -> torch.Tensor:
    """eps = WaveNet((audio [B,1,L], t * ones)) on the engine, differentiable in `audio` (WaveNetEpsHIP)."""
    return WaveNetEpsHIP.apply(audio, engine, int(t))


class WaveNetEpsLenHIP(torch.autograd.Function):
    """WaveNetEpsHIP for clips of any length <= engine.L (audio [B,1,len]): wavenet_eps_len forward, wavenet_eps_vjp_len backward,
    both on the exact-fp32 path whatever the engine's mode.  First-order only: create_graph=True raises."""

    @staticmethod
    def forward(ctx, audio, engine, t):
        from . import engine as _eng
        _require_cuda(audio)
        if engine.precision not in (_eng.FP32, _eng.EXACT):
            raise DmadError('the HIP VJP runs on the exact-fp32 path: a BF16 engine holds no fp32 weights (use an FP32 or EXACT engine)')
        eps = engine.wavenet_eps_len(audio, t)
        ctx.engine, ctx.t = engine, int(t)
        ctx.save_for_backward(audio)
        return eps.view(audio.shape)

    @staticmethod
    def backward(ctx, g_eps):
        _first_order_only('WaveNet')
        audio, = ctx.saved_tensors
        eng, B = ctx.engine, audio.shape[0]
        if eng.vjp_batch < B:
            eng.reserve_vjp(B)
        g_x = eng.wavenet_eps_vjp_len(audio, ctx.t, g_eps.reshape(audio.shape).contiguous())
        return g_x.view(audio.shape).to(audio.dtype), None, None


def wavenet_eps_len_hip(engine, audio: torch.Tensor, t: int) -> torch.Tensor:
    """eps = WaveNet((audio [B,1,len], t * ones)) for len <= engine.L on the engine, differentiable in `audio` (WaveNetEpsLenHIP)."""
    return WaveNetEpsLenHIP.apply(audio, engine, int(t))


def has_unet_vjp(engine) -> bool:
    """The engine holds the exact-fp32 UNet tier as a product path (FP32 and EXACT engines), the tier UNetEpsHIP runs on."""
    from . import engine as _eng
    return getattr(engine, 'precision', None) in (_eng.FP32, _eng.EXACT)


class UNetEpsHIP(torch.autograd.Function):
    """eps = UNetModel(x [B,1,32,32], t * ones) on the engine's exact-fp32 UNet tier, differentiable in `x` through the engine's VJP.
    Saves only the input; the backward re-runs the forward with its tape saved (dmad_unet_eps_vjp).  The VJP workspace is reserved
    on first use.  First-order only: create_graph=True raises."""

    @staticmethod
    def forward(ctx, x, engine, t):
        _require_cuda(x)
        if not has_unet_vjp(engine):
            raise DmadError('the HIP UNet VJP runs on the exact-fp32 UNet tier: use an FP32 or EXACT engine')
        eps = engine.unet_eps(x, t, tier=0)
        ctx.engine, ctx.t = engine, int(t)
        ctx.save_for_backward(x)
        return eps.view(x.shape)

    @staticmethod
    def backward(ctx, g_eps):
        _first_order_only('UNet', torch_hint=False)
        x, = ctx.saved_tensors
        eng, B = ctx.engine, x.shape[0]
        if eng.unet_vjp_batch < B:
            eng.reserve_unet_vjp(B)
        g_x = eng.unet_eps_vjp(x, ctx.t, g_eps.reshape(x.shape).contiguous())
        return g_x.view(x.shape).to(x.dtype), None, None


def unet_eps_hip(engine, x: torch.Tensor, t: int) -> torch.Tensor:
    """eps = UNetModel(x [B,1,32,32], t * ones) on the engine, differentiable in `x` (UNetEpsHIP)."""
    return UNetEpsHIP.apply(x, engine, int(t))


def _classifier_forward(ctx, spec, engine):
    """the forward of ResNeXtHIP, VGGHIP, WRNHIP and DNHIP: the resident classifier's fp32 tier"""
    _require_cuda(spec)
    logits = engine.classify_tier(spec, 0)
    ctx.engine = engine
    ctx.save_for_backward(spec)
    return logits


class ResNeXtHIP(torch.autograd.Function):
    """logits = CifarResNeXt(spec [B,1,32,32]) on the engine's fp32 ResNeXt29 tier (classify_tier(spec, 0)), differentiable in `spec`
    through the engine's VJP.  Saves only the input; the backward re-runs the forward with its tape saved (dmad_classify_vjp).  The VJP
    workspace is reserved on first use.  No weight gradients.  First-order only: create_graph=True raises."""
    forward = staticmethod(_classifier_forward)

    @staticmethod
    def backward(ctx, g_logits):
        _first_order_only('ResNeXt29')
        spec, = ctx.saved_tensors
        eng, B = ctx.engine, spec.shape[0]
        if eng.classifier_vjp_batch < B:
            eng.reserve_classifier_vjp(B)
        g = eng.classify_vjp(spec, g_logits.contiguous())
        return g.view(spec.shape).to(spec.dtype), None


def resnext_hip(engine, spec: torch.Tensor) -> torch.Tensor:
    """logits = CifarResNeXt(spec [B,1,32,32]) on the engine's fp32 tier, differentiable in `spec` (ResNeXtHIP)."""
    return ResNeXtHIP.apply(spec, engine)


class VGGHIP(torch.autograd.Function):
    """logits = VGG19_bn(spec [B,1,32,32]) on the engine's fp32 tier (classify_tier(spec, 0)), differentiable in `spec` through the
    engine's VJP.  Saves only the input; the backward re-runs the forward with its tape saved (dmad_vgg_vjp).  The VJP workspace is
    reserved on first use.  No weight gradients.  First-order only: create_graph=True raises."""
    forward = staticmethod(_classifier_forward)

    @staticmethod
    def backward(ctx, g_logits):
        _first_order_only('VGG19_bn')
        spec, = ctx.saved_tensors
        eng, B = ctx.engine, spec.shape[0]
        if eng.vgg_vjp_batch < min(B, eng.max_batch):
            eng.reserve_vgg_vjp(B)
        g = eng.vgg_vjp(spec, g_logits.contiguous())
        return g.view(spec.shape).to(spec.dtype), None


def vgg_hip(engine, spec: torch.Tensor) -> torch.Tensor:
    """logits = VGG19_bn(spec [B,1,32,32]) on the engine's fp32 tier, differentiable in `spec` (VGGHIP)."""
    return VGGHIP.apply(spec, engine)


class WRNHIP(torch.autograd.Function):
    """logits = WideResNet-28-10(spec [B,1,32,32]) on the engine's fp32 tier (classify_tier(spec, 0)), differentiable in `spec` through
    the engine's VJP.  Saves only the input; the backward re-runs the forward with its tape saved (dmad_wrn_vjp).  The VJP workspace is
    reserved on first use.  No weight gradients.  First-order only: create_graph=True raises."""
    forward = staticmethod(_classifier_forward)

    @staticmethod
    def backward(ctx, g_logits):
        _first_order_only('WideResNet-28-10')
        spec, = ctx.saved_tensors
        eng, B = ctx.engine, spec.shape[0]
        if eng.wrn_vjp_batch < min(B, eng.max_batch):
            eng.reserve_wrn_vjp(B)
        g = eng.wrn_vjp(spec, g_logits.contiguous())
        return g.view(spec.shape).to(spec.dtype), None


def wrn_hip(engine, spec: torch.Tensor) -> torch.Tensor:
    """logits = WideResNet-28-10(spec [B,1,32,32]) on the engine's fp32 tier, differentiable in `spec` (WRNHIP)."""
    return WRNHIP.apply(spec, engine)


class DNHIP(torch.autograd.Function):
    """logits = DenseNet-BC-100-12(spec [B,1,32,32]) on the engine's fp32 tier (classify_tier(spec, 0)), differentiable in `spec` through
    the engine's VJP.  Saves only the input; the backward re-runs the forward with its tape saved (dmad_dn_vjp).  The VJP workspace is
    reserved on first use.  No weight gradients.  First-order only: create_graph=True raises."""
    forward = staticmethod(_classifier_forward)

    @staticmethod
    def backward(ctx, g_logits):
        _first_order_only('DenseNet-BC-100-12')
        spec, = ctx.saved_tensors
        eng, B = ctx.engine, spec.shape[0]
        if eng.dn_vjp_batch < min(B, eng.max_batch):
            eng.reserve_dn_vjp(B)
        g = eng.dn_vjp(spec, g_logits.contiguous())
        return g.view(spec.shape).to(spec.dtype), None


def dn_hip(engine, spec: torch.Tensor) -> torch.Tensor:
    """logits = DenseNet-BC-100-12(spec [B,1,32,32]) on the engine's fp32 tier, differentiable in `spec` (DNHIP)."""
    return DNHIP.apply(spec, engine)


class M5HIP(torch.autograd.Function):
    """log-probabilities = M5(x [B,1,L]) on the engine (m5_logits), differentiable in `x` through the engine's VJP (dmad_m5_vjp, which
    recomputes the forward and keeps only the pool / ReLU decisions).  Saves only the input; nothing is reserved.  No weight gradients.
    First-order only: create_graph=True raises."""

    @staticmethod
    def forward(ctx, x, engine):
        _require_cuda(x)
        ctx.engine = engine
        ctx.save_for_backward(x)
        return engine.m5_logits(x)

    @staticmethod
    def backward(ctx, g_logp):
        _first_order_only('M5')
        x, = ctx.saved_tensors
        g = ctx.engine.m5_vjp(x, g_logp.contiguous())
        return g.view(x.shape).to(x.dtype), None


def m5_hip(engine, x: torch.Tensor) -> torch.Tensor:
    """log-probabilities = M5(x [B,1,L]) on the engine, differentiable in `x` (M5HIP)."""
    return M5HIP.apply(x, engine)


class MelDBHIP(torch.autograd.Function):
    """[B,1,16000] -> [B,1,32,32] dB mel spectrogram on the engine (mel_db), differentiable in `x` through the engine's mel VJP
    (dmad_mel_db_vjp, which recomputes the forward).  Saves only the input.  First-order only: create_graph=True raises."""

    @staticmethod
    def forward(ctx, x, engine):
        _require_cuda(x)
        ctx.engine = engine
        ctx.save_for_backward(x)
        return engine.mel_db(x)

    @staticmethod
    def backward(ctx, g_spec):
        _first_order_only('mel')
        x, = ctx.saved_tensors
        g = ctx.engine.mel_db_vjp(x, g_spec.contiguous())
        return g.view(x.shape).to(x.dtype), None


def mel_db_hip(engine, x: torch.Tensor) -> torch.Tensor:
    """[B,1,16000] -> [B,1,32,32] dB mel spectrogram on the engine, differentiable in x (MelDBHIP)."""
    return MelDBHIP.apply(x, engine)


class WaveSmoothHIP(torch.autograd.Function):
    """[B,L] -> [B,L] zero-padded windowed mean (kind 0, AS) or median (kind 1, MS) on the engine (wave_smooth); the backward is the
    engine's VJP (dmad_wave_smooth_vjp: the mean is its own transpose, the median routes by the lowest-position rule)."""

    @staticmethod
    def forward(ctx, x, engine, kind, window):
        _require_cuda(x)
        ctx.engine, ctx.kind, ctx.window = engine, int(kind), int(window)
        ctx.save_for_backward(x)
        return engine.wave_smooth(x, kind, window)

    @staticmethod
    def backward(ctx, g_y):
        x, = ctx.saved_tensors
        g = ctx.engine.wave_smooth_vjp(x, g_y.contiguous(), ctx.kind, ctx.window)
        return g.view(x.shape).to(x.dtype), None, None, None


class WaveResampleHIP(torch.autograd.Function):
    """[B,L_in] -> [B,L_out] polyphase FIR resampling on the engine (wave_resample); the backward is the transposed operator
    (dmad_wave_resample_vjp)."""

    @staticmethod
    def forward(ctx, x, engine, ker, stride, width, L_out):
        _require_cuda(x)
        ctx.engine, ctx.ker, ctx.stride, ctx.width, ctx.L_in = engine, ker, int(stride), int(width), x.shape[-1]
        return engine.wave_resample(x, ker, stride, width, L_out)

    @staticmethod
    def backward(ctx, g_y):
        g = ctx.engine.wave_resample_vjp(g_y.contiguous(), ctx.L_in, ctx.ker, ctx.stride, ctx.width)
        return g.to(g_y.dtype), None, None, None, None, None


class WaveIIRHIP(torch.autograd.Function):
    """[B,L] -> clamp(lfilter(b, a, x), lo, hi) on the engine (wave_iir); the backward is the flipped filter on the masked gradient
    (dmad_wave_iir_vjp, which recomputes the forward for the mask)."""

    @staticmethod
    def forward(ctx, x, engine, b, a, lo, hi):
        _require_cuda(x)
        ctx.engine, ctx.b, ctx.a, ctx.lo, ctx.hi = engine, b, a, float(lo), float(hi)
        ctx.save_for_backward(x)
        return engine.wave_iir(x, b, a, lo, hi)

    @staticmethod
    def backward(ctx, g_y):
        x, = ctx.saved_tensors
        g = ctx.engine.wave_iir_vjp(x, g_y.contiguous(), ctx.b, ctx.a, ctx.lo, ctx.hi)
        return g.view(x.shape).to(x.dtype), None, None, None, None, None


class KWSHIP(torch.autograd.Function):
    """log-probabilities = KWSModel(spec [B,1,32,T]) on the engine (kws_logits), differentiable in `spec` through the engine's VJP
    (dmad_kws_vjp, which recomputes the forward and walks back through time in the same launch).  Saves only the input; nothing is
    reserved.  No weight gradients.  First-order only: create_graph=True raises."""

    @staticmethod
    def forward(ctx, spec, engine):
        _require_cuda(spec)
        ctx.engine = engine
        ctx.save_for_backward(spec)
        return engine.kws_logits(spec)

    @staticmethod
    def backward(ctx, g_logp):
        _first_order_only('KWS')
        spec, = ctx.saved_tensors
        g = ctx.engine.kws_vjp(spec, g_logp.contiguous())
        return g.view(spec.shape).to(spec.dtype), None


def kws_hip(engine, spec: torch.Tensor) -> torch.Tensor:
    """log-probabilities = KWSModel(spec [B,1,32,T] or [B,32,T]) on the engine, differentiable in `spec` (KWSHIP)."""
    return KWSHIP.apply(spec, engine)


_KWS_MEL_CACHE = {}


def kws_mel_filterbank() -> np.ndarray:
    """The htk filterbank of torchaudio MelSpectrogram(sample_rate=16000, n_mels=32) in float64, [32][201]: 34 points equally spaced in
    mel = 2595 log10(1 + f / 700) between 0 and 8000 Hz, bins at linspace(0, 8000, 201), max(0, min(down, up)), no norm."""
    mel = np.linspace(0.0, 2595.0 * np.log10(1.0 + 8000.0 / 700.0), 34)
    pts = 700.0 * (10.0 ** (mel / 2595.0) - 1.0)
    freqs = np.linspace(0.0, 8000.0, 201)
    down = (freqs[None, :] - pts[:-2, None]) / (pts[1:-1, None] - pts[:-2, None])
    up = (pts[2:, None] - freqs[None, :]) / (pts[2:, None] - pts[1:-1, None])
    return np.maximum(0.0, np.minimum(down, up))


def kws_mel_db(x: torch.Tensor) -> torch.Tensor:
    """[B,1,L] -> [B,1,32,1 + L // 200] dB mel spectrogram of the keyword spotter's front-end (torchaudio MelSpectrogram(16000,
    n_mels=32) then AmplitudeToDB('power')), differentiable in x, in x's dtype and on x's device: the restatement in torch ops that the
    CPU path and the grad_backend = 'torch' branch run (the engine's kernels are dmad_kws_mel_*)."""
    key = (str(x.device), x.dtype)
    if key not in _KWS_MEL_CACHE:
        _KWS_MEL_CACHE[key] = (torch.hann_window(400, periodic=True, dtype=torch.float64).to(x.device, x.dtype),
                               torch.from_numpy(kws_mel_filterbank()).to(x.device, x.dtype))
    win, fb = _KWS_MEL_CACHE[key]
    spec = torch.stft(x[:, 0], n_fft=400, hop_length=200, win_length=400, window=win, center=True, pad_mode='reflect',
                      normalized=False, onesided=True, return_complex=True)
    power = spec.real ** 2 + spec.imag ** 2                                        # [B, 201, T]
    mel = torch.matmul(fb, power)                                                  # [B, 32, T]
    return (10.0 * torch.log10(torch.clamp(mel, min=1e-10))).unsqueeze(1)


class KWSMelDBHIP(torch.autograd.Function):
    """[B,1,L] -> [B,1,32,T] dB mel spectrogram of the keyword spotter's front-end on the engine (kws_mel_db), differentiable in `x`
    through the engine's VJP (dmad_kws_mel_db_vjp, which recomputes the forward).  Saves only the input.  First-order only:
    create_graph=True raises."""

    @staticmethod
    def forward(ctx, x, engine):
        _require_cuda(x)
        ctx.engine = engine
        ctx.save_for_backward(x)
        return engine.kws_mel_db(x).unsqueeze(1)

    @staticmethod
    def backward(ctx, g_spec):
        _first_order_only('KWS mel')
        x, = ctx.saved_tensors
        g = ctx.engine.kws_mel_db_vjp(x, g_spec.contiguous())
        return g.view(x.shape).to(x.dtype), None


def kws_mel_db_hip(engine, x: torch.Tensor) -> torch.Tensor:
    """[B,1,L] -> [B,1,32,T] on the engine, differentiable in x (KWSMelDBHIP)."""
    return KWSMelDBHIP.apply(x, engine)


class KWSWaveHIP(torch.autograd.Function):
    """log-probabilities = KWSModel(kws_mel_db(x [B,1,L])) on the engine in one call (kws_wave_logits: only the frames the model reads
    are computed), differentiable in `x` through dmad_kws_wave_vjp (the KWS VJP, then the mel VJP on the read frames).  Saves only the
    input; nothing is reserved.  No weight gradients.  First-order only: create_graph=True raises."""

    @staticmethod
    def forward(ctx, x, engine):
        _require_cuda(x)
        ctx.engine = engine
        ctx.save_for_backward(x)
        return engine.kws_wave_logits(x)

    @staticmethod
    def backward(ctx, g_logp):
        _first_order_only('KWS wave')
        x, = ctx.saved_tensors
        g = ctx.engine.kws_wave_vjp(x, g_logp.contiguous())
        return g.view(x.shape).to(x.dtype), None


def kws_wave_hip(engine, x: torch.Tensor) -> torch.Tensor:
    """log-probabilities = KWSModel(kws_mel_db(x)) on the engine, differentiable in `x` (KWSWaveHIP)."""
    return KWSWaveHIP.apply(x, engine)
