"""Host mirror of the reference's diffusion_models/diffwave_sde.py — the reverse VP-SDE DiffWave purifier that the adaptive-attack
driver builds for `--defense Diffusion` (adaptive_attack_eval.py) — backed by the MI355X engine (libdmad_hip.so).  Same names,
constructor signatures and attributes as the reference:

  RevVPSDE(model, score_type='ddpm', beta_min=0.02, beta_max=4, N=200, audio_shape=(1, 16000), model_kwargs=None)
      .discrete_betas / .alphas_cumprod / .sqrt_1m_alphas_cumprod / .noise_type / .sde_type,
      ._scale_timesteps / .vpsde_fn / .rvpsde_fn / .f(t, x) / .g(t, x) on [B, L] tensors
  RevDiffWave(args, device=None) .T / .model / .rev_vpsde / .betas, .audio_editing_sample(audio), .forward(x)

The reference integrates the reverse SDE with torchsde.sdeint_adjoint (Euler, dt = 1/T).  torchsde is not used here: at a fixed
step its loop is a short chain, and this module owns it.  `vpsde_schedule` restates that loop in float32 and in torchsde's order
(next_t = min(curr_t + dt, ts[-1]); the step index k = long((1 - curr_t) * N)), which repeats and skips indices; the
chain then runs as one library call (dmad_vpsde_purify):  x <- c_a x0 + c_b z;  x <- x + (beta/2 x - q eps_k(x)) h + gs z  per step.

Noise: on-device Philox keyed (seed, sample0 + row) like DiffWave's noise_source='device' — stream 0x5DE00000 for the diffusion draw,
0x5DE00001 + n for Euler step n; row i of a call is sample `_draws + i`, and every round of sample_step takes the next B samples.
`use_bm` is accepted and changes nothing: both settings draw the Brownian increments from Philox, and torchsde's Brownian stream
(BrownianInterval or its default) is not reproduced.

Gradients (RevDiffWave(..., score_grad=...)):
  'none'  (default) the reference's semantics.  The reference's DiffWave.compute_eps_t is decorated @torch.no_grad(), so the
          adjoint sees eps as a constant and the attack gradient is a scalar times g_out.  Here the forward is the inference chain
          (attack and evaluation forwards are bit-identical) and the backward is c_a * prod(1 + h beta/2) * g_out, the exact derivative
          of the executed chain with eps held constant (the reference's adjoint matches it up to O(h)).
  'hip'   the full gradient of the chain, eps-network included: the forward runs on the exact-fp32 path and keeps the trajectory
          (S + 1 states of B x L), the backward is one library call (dmad_vpsde_purify_vjp).  FP32 / EXACT engines.
  'torch' the same full gradient composed from dmad_hip.autograd.wavenet_eps with the same Philox draws (the cross-check; needs the
          state dict; allocator-hungry).
'none' and 'hip' are first-order only: create_graph=True raises DmadError, as WaveNetEpsHIP does."""
from typing import NamedTuple

import numpy as np
import torch

from dmad_hip import autograd as _ag
from dmad_hip import engine as _eng
from dmad_hip._lib import DmadError
from .diffwave_ddpm import DiffWave, create_diffwave_model

VPSDE_STREAM_DIFFUSE = 0x5DE00000          # Philox stream of the diffusion draw (include/dmad.h dmad_vpsde_purify)
VPSDE_STREAM_STEP0 = 0x5DE00001            # ... of Euler step n: VPSDE_STREAM_STEP0 + n
SCORE_GRADS = ('none', 'hip', 'torch')


def _extract_into_tensor(arr_or_func, timesteps, broadcast_shape):
    """A table (tensor) or a callable, indexed by `timesteps`, broadcast to the shape (same helper as the reference's)."""
    if callable(arr_or_func):
        res = arr_or_func(timesteps).float()
    else:
        res = arr_or_func.to(device=timesteps.device)[timesteps].float()
    while len(res.shape) < len(broadcast_shape):
        res = res[..., None]
    return res.expand(broadcast_shape)


class VPSDESchedule(NamedTuple):
    """Per Euler step n: k[n] (step index of the eps-network), h[n] (step length), hb[n] (beta/2), q[n] ((sqrt beta)^2 / sqrt(1 - abar_k)),
    gs[n] (scale_factor * sqrt(beta) * sqrt(h)); c_a / c_b of the initial diffusion.  float32 values (k int32)."""
    k: np.ndarray
    h: np.ndarray
    hb: np.ndarray
    q: np.ndarray
    gs: np.ndarray
    c_a: float
    c_b: float

    @property
    def steps(self) -> int:
        return len(self.k)

    def linear_gain(self) -> float:
        """c_a * prod(1 + h beta/2): d out / d x0 of the chain with eps held constant (the 'none' gradient), in float64."""
        return float(np.float64(self.c_a) * np.prod(1.0 + self.h.astype(np.float64) * self.hb.astype(np.float64)))


def vpsde_schedule(t: int, T: int = 200, N: int = 200, betas=None, beta_min=None, beta_max=None, t_diffuse=None) -> VPSDESchedule:
    """The Euler steps of RevDiffWave.audio_editing_sample's sdeint_adjoint(RevVPSDE, ts = linspace(1 - t/T, 1 - 1e-5, 2), 'euler',
    dt = 1/T), computed on the host in float32 and in the reference's order.  betas: the RevVPSDE's discrete_betas (default
    linspace(beta_min/N, beta_max/N, N)); beta_min / beta_max: its beta_0 / beta_1 (default 0.0001 T / 0.02 T, RevDiffWave's).
    t_diffuse: the noise level of the initial diffusion (c_a, c_b); the reference's rand_t changes it and keeps the integration range
    at t (default t)."""
    beta_0 = 0.0001 * T if beta_min is None else beta_min
    beta_1 = 0.02 * T if beta_max is None else beta_max
    if betas is None:
        betas = torch.linspace(beta_0 / N, beta_1 / N, N)
    betas = torch.as_tensor(betas).detach().cpu().float()
    alphas_cumprod = torch.cumprod(1. - betas, dim=0)
    sqrt_1m = torch.sqrt(1. - alphas_cumprod)
    td = t if t_diffuse is None else int(t_diffuse)
    if not 1 <= td <= len(betas):
        raise ValueError('diffusion level %d outside [1, %d]' % (td, len(betas)))
    a = (1 - betas).cumprod(dim=0)
    c_a, c_b = float(a[td - 1].sqrt()), float((1.0 - a[td - 1]).sqrt())
    ts = torch.linspace(1 - t / T, 1 - 1e-5, 2)
    curr, end, dt = ts[0], ts[-1], 1. / T
    k, h, hb, q, gs = [], [], [], [], []
    while curr < end:                                   # torchsde's fixed-step loop (base_solver.integrate)
        nxt = min(curr + dt, end)
        tt = 1 - curr.reshape(1)                        # RevVPSDE.f / g evaluate at 1 - t, the start of the step
        kk = int((tt.float() * N).long()[0])            # _scale_timesteps
        if not 0 <= kk < N:
            raise ValueError('step index %d outside [0, %d) at t = %d' % (kk, N, t))
        beta_t = beta_0 + (tt * N - 1) / (N - 1) * (beta_1 - beta_0)          # vpsde_fn
        diffusion = torch.sqrt(beta_t)
        scale = torch.sqrt(1 - alphas_cumprod[kk - 1]) / torch.sqrt(1 - alphas_cumprod[kk]) if kk > 0 else torch.zeros(())
        step = nxt - curr
        k.append(kk)
        h.append(float(step))
        hb.append(float((0.5 * beta_t)[0]))
        q.append(float((diffusion ** 2 / sqrt_1m[kk])[0]))
        gs.append(float((scale * diffusion * torch.sqrt(step))[0]))
        curr = nxt
    f32 = lambda v: np.asarray(v, dtype=np.float32)     # noqa: E731
    return VPSDESchedule(np.asarray(k, dtype=np.int32), f32(h), f32(hb), f32(q), f32(gs), c_a, c_b)


class RevVPSDE(torch.nn.Module):
    """The reverse VP-SDE of the reference (drift -f(x, 1 - t), diffusion g(1 - t)) on [B, L] tensors, with the score from the DiffWave
    mirror's eps-network.  RevDiffWave does not integrate it op by op: its chain runs on the engine (vpsde_schedule)."""

    def __init__(self, model: DiffWave, score_type='ddpm', beta_min=0.02, beta_max=4, N=200, audio_shape=(1, 16000), model_kwargs=None):
        super().__init__()
        self.model = model
        self.score_type = score_type
        self.model_kwargs = model_kwargs
        self.audio_shape = audio_shape
        self.beta_0 = beta_min
        self.beta_1 = beta_max
        self.N = N
        self.discrete_betas = torch.linspace(beta_min / N, beta_max / N, N)
        self.alphas = 1. - self.discrete_betas
        self.alphas_cumprod = torch.cumprod(self.alphas, dim=0)
        self.sqrt_alphas_cumprod = torch.sqrt(self.alphas_cumprod)
        self.sqrt_1m_alphas_cumprod = torch.sqrt(1. - self.alphas_cumprod)
        self.alphas_cumprod_cont = lambda t: torch.exp(-0.5 * (self.beta_1 - self.beta_0) * t ** 2 - self.beta_0 * t)
        self.sqrt_1m_alphas_cumprod_neg_recip_cont = lambda t: -1. / torch.sqrt(1. - self.alphas_cumprod_cont(t))
        self.noise_type = "diagonal"
        self.sde_type = "ito"

    def _scale_timesteps(self, t):
        assert torch.all(t <= 1) and torch.all(t >= 0), f't has to be in [0, 1], but get {t} with shape {t.shape}'
        return (t.float() * self.N).long()

    def vpsde_fn(self, t, x):
        beta_t = self.beta_0 + (t * self.N - 1) / (self.N - 1) * (self.beta_1 - self.beta_0)
        drift = -0.5 * beta_t[:, None] * x
        diffusion = torch.sqrt(beta_t)
        return drift, diffusion

    def rvpsde_fn(self, t, x, return_type='drift'):
        """Drift (return_type='drift') or diffusion of the reverse SDE at time t (shape [B])."""
        drift, diffusion = self.vpsde_fn(t, x)
        if return_type == 'drift':
            assert x.ndim == 2 and np.prod(self.audio_shape) == x.shape[1], x.shape
            x_audio = x.view(-1, *self.audio_shape)
            if self.score_type != 'guided_diffusion':
                raise NotImplementedError(f'Unknown score type in RevVPSDE: {self.score_type}!')
            disc_steps = self._scale_timesteps(t)
            with torch.no_grad():                        # the reference's compute_eps_t is @torch.no_grad()
                epsilon_theta = self.model.compute_eps_t(x_audio, int(disc_steps[0]))
            assert x_audio.shape == epsilon_theta.shape, f'{x_audio.shape}, {epsilon_theta.shape}'
            epsilon_theta = epsilon_theta.view(x.shape[0], -1)
            score = - epsilon_theta / self.sqrt_1m_alphas_cumprod[disc_steps[0]].to(x.device)
            return drift - diffusion[:, None] ** 2 * score
        disc_steps = self._scale_timesteps(t)
        if disc_steps.unique() > 0:
            scale_factor = torch.sqrt(1 - self.alphas_cumprod[disc_steps - 1]) / torch.sqrt(1 - self.alphas_cumprod[disc_steps])
            scale_factor = scale_factor.to(x.device)
        else:
            scale_factor = 0
        return scale_factor * diffusion

    def f(self, t, x):
        """The drift -f(x, 1 - t) of the time-reversed SDE (t' = 1 - t), on [B, L]."""
        t = t.expand(x.shape[0])
        drift = self.rvpsde_fn(1 - t, x, return_type='drift')
        assert drift.shape == x.shape
        return -drift

    def g(self, t, x):
        """The diffusion g(1 - t), broadcast to [B, L]."""
        t = t.expand(x.shape[0])
        diffusion = self.rvpsde_fn(1 - t, x, return_type='diffusion')
        assert diffusion.shape == (x.shape[0], )
        return diffusion[:, None].expand(x.shape)


class _ChainNone(torch.autograd.Function):
    """score_grad='none': the inference chain forward; backward = c_a prod(1 + h beta/2) g_out (eps held constant)."""

    @staticmethod
    def forward(ctx, x0, den, sch, sample0):
        ctx.gain = sch.linear_gain()
        return den._run(x0, sch, sample0, path=0).view(x0.shape)

    @staticmethod
    def backward(ctx, g_out):
        if torch.is_grad_enabled():
            raise DmadError("the VP-SDE chain's gradient is first-order only: create_graph=True (double backward) is not supported; "
                            "use score_grad='torch' for higher derivatives")
        return g_out * ctx.gain, None, None, None


class _ChainHIP(torch.autograd.Function):
    """score_grad='hip': the exact-fp32 chain, its trajectory kept; backward = dmad_vpsde_purify_vjp."""

    @staticmethod
    def forward(ctx, x0, den, sch, sample0):
        eng = den.engine
        out, traj = eng.vpsde_purify(x0, sch.c_a, sch.c_b, sch.k, sch.h, sch.hb, sch.q, sch.gs, seed=den.seed, sample0=sample0, path=1,
                                     want_traj=True)
        ctx.engine, ctx.sch = eng, sch
        ctx.save_for_backward(traj)
        return out.view(x0.shape)

    @staticmethod
    def backward(ctx, g_out):
        if torch.is_grad_enabled():
            raise DmadError("the HIP VP-SDE gradient is first-order only: create_graph=True (double backward) is not supported; "
                            "use score_grad='torch' for higher derivatives")
        traj, = ctx.saved_tensors
        eng, sch = ctx.engine, ctx.sch
        B = g_out.shape[0]
        if getattr(eng, 'vjp_batch', 0) < min(B, eng.max_batch):
            eng.reserve_vjp(min(B, eng.max_batch))
        g = eng.vpsde_purify_vjp(traj, sch.c_a, sch.k, sch.h, sch.hb, sch.q, g_out.reshape(B, -1).contiguous())
        return g.view(g_out.shape).to(g_out.dtype), None, None, None


class RevDiffWave(torch.nn.Module):
    """The reference's RevDiffWave (explicitly adapted for DiffWave).  Reads args.ddpm_path, ddpm_config, t, score_type, sample_step,
    rand_t, t_delta and use_bm.  Keywords beyond the reference's: state_dict / engine / precision / max_batch (passed to
    create_diffwave_model; synthetic weights), score_grad ('none' | 'hip' | 'torch', see the module docstring), seed (Philox key)."""

    def __init__(self, args, device=None, score_grad='none', seed=0, **kw):
        super().__init__()
        self.args = args
        if device is None:
            device = torch.device("cuda") if torch.cuda.is_available() else torch.device("cpu")
        self.device = device
        audio_shape = (1, 16000)
        extra = {key: kw.pop(key) for key in ('state_dict', 'engine', 'precision', 'max_batch') if key in kw}
        if kw:
            raise TypeError('unexpected keyword arguments %s' % sorted(kw))
        model = create_diffwave_model(model_path=args.ddpm_path, config_path=args.ddpm_config, reverse_timestep=args.t, **extra)
        model.eval()
        self.T = 200
        self.model = model
        self.rev_vpsde = RevVPSDE(model=model, score_type=args.score_type, beta_min=0.0001 * self.T, beta_max=0.02 * self.T, N=self.T,
                                  audio_shape=audio_shape, model_kwargs=None)
        self.betas = self.rev_vpsde.discrete_betas.float()
        self.score_grad = score_grad
        self.seed = int(seed)
        self._draws = 0
        if score_grad == 'hip' and self.engine.precision == _eng.BF16:
            raise DmadError("score_grad='hip' runs the chain on the exact-fp32 path: a BF16 engine holds no fp32 weights "
                            '(use an FP32 or EXACT engine)')

    @property
    def score_grad(self) -> str:
        return self._score_grad

    @score_grad.setter
    def score_grad(self, value: str):
        if value not in SCORE_GRADS:
            raise ValueError('score_grad must be one of %s, not %r' % (SCORE_GRADS, value))
        self._score_grad = value

    @property
    def engine(self) -> "_eng.Engine":
        return self.model.engine

    def schedule(self, t_diffuse=None) -> VPSDESchedule:
        """The Euler steps of one round at args.t (the initial diffusion at t_diffuse, default args.t)."""
        return vpsde_schedule(self.args.t, self.T, self.T, self.rev_vpsde.discrete_betas, self.rev_vpsde.beta_0, self.rev_vpsde.beta_1,
                              t_diffuse=t_diffuse)

    def _run(self, x0, sch, sample0, path):
        """One chain on the engine, no gradient: [B, 1, L] -> [B, L]."""
        return self.engine.vpsde_purify(x0, sch.c_a, sch.c_b, sch.k, sch.h, sch.hb, sch.q, sch.gs, seed=self.seed, sample0=sample0, path=path)

    def _run_torch(self, x0, sch, sample0):
        """The chain composed from the torch restatement of the eps-network, with the engine's Philox draws."""
        folded = self.model.model._folded
        if folded is None:
            raise DmadError("score_grad='torch' needs the torch restatement: build the model with its state dict")
        eng, B = self.engine, x0.shape[0]
        x = x0.reshape(B, -1)
        x = sch.c_a * x + sch.c_b * eng.philox_normal(self.seed, sample0, VPSDE_STREAM_DIFFUSE, B)
        for n in range(sch.steps):
            eps = _ag.wavenet_eps(folded, x.unsqueeze(1), int(sch.k[n]))[:, 0]
            x = x + (float(sch.hb[n]) * x - float(sch.q[n]) * eps) * float(sch.h[n])
            if sch.gs[n] != 0:
                x = x + float(sch.gs[n]) * eng.philox_normal(self.seed, sample0, VPSDE_STREAM_STEP0 + n, B)
        return x.view(x0.shape)

    def _chain(self, x0, sch):
        sample0 = self._draws
        self._draws += x0.shape[0]
        grad = _ag.needs_grad(x0)
        if self._score_grad == 'torch' and grad:
            return self._run_torch(x0, sch, sample0)
        if self._score_grad == 'hip':
            if grad:
                return _ChainHIP.apply(x0, self, sch, sample0)
            with torch.no_grad():
                return self._run(x0, sch, sample0, path=1).view(x0.shape)
        if grad:
            return _ChainNone.apply(x0, self, sch, sample0)
        with torch.no_grad():
            return self._run(x0, sch, sample0, path=0).view(x0.shape)

    def audio_editing_sample(self, audio):
        """audio in [-1, 1], [B, 1, L]: sample_step rounds of (diffuse to t, reverse VP-SDE chain), each round's output the next one's
        input, the rounds concatenated on dim 0."""
        assert isinstance(audio, torch.Tensor)
        assert audio.ndim == 3, audio.ndim
        x0 = audio.to(self.device)
        if self.rev_vpsde.score_type != 'guided_diffusion':     # the reference raises when sdeint first evaluates the drift
            raise NotImplementedError(f'Unknown score type in RevVPSDE: {self.rev_vpsde.score_type}!')
        xs = []
        for _ in range(self.args.sample_step):
            total_noise_levels = self.args.t
            if self.args.rand_t:
                total_noise_levels = self.args.t + np.random.randint(-self.args.t_delta, self.args.t_delta)
            x0 = self._chain(x0, self.schedule(total_noise_levels))
            xs.append(x0)
        return torch.cat(xs, dim=0)

    def forward(self, x):
        return self.audio_editing_sample(x)
