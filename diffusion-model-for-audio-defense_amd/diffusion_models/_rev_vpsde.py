"""What the two reverse VP-SDE purifiers (diffwave_sde.RevDiffWave on waveforms, improved_diffusion_sde.RevImprovedDiffusion on mel
spectrograms) share on the host.  Private: the reference has no such module, and torchsde is not used here.

  VPSDESchedule, euler_schedule   the Euler steps of the reference's sdeint_adjoint call, restated in float32 and in torchsde's order
  RevVPSDEBase                    the reference RevVPSDE's tables, _scale_timesteps, f and g; each module's RevVPSDE adds its own
                                  constructor signature, vpsde_fn and rvpsde_fn
  _ChainNone, _ChainHIP           the chain as an autograd function: eps held constant / the full gradient from the engine
  ChainPurifier                   score_grad, engine, the dispatch over score_grad (_chain) and the sample_step rounds (_rounds)

A purifier built on ChainPurifier provides args, rev_vpsde, model (with .engine), seed, _draws, its SCORE_GRADS tuple and
  schedule(t_diffuse) -> VPSDESchedule
  _run(x0, sch, sample0, path, want_traj=False)   one chain on the engine: path 0 the mode's default, 1 exact fp32
  _run_vjp(traj, sch, g_out)                      the reverse walk over the trajectory of _run(.., path=1, want_traj=True)
  _run_torch(x0, sch, sample0)                    the chain composed from torch ops, with the engine's Philox draws"""
from typing import NamedTuple

import numpy as np
import torch

from dmad_hip._lib import DmadError
from dmad_hip.autograd import needs_grad


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
    """Per Euler step n: k[n] (step index of the eps-network), h[n] (step length), hb[n] (beta/2), q[n] ((sqrt beta)^2 / sqrt(1 - abar)),
    gs[n] (noise scale times sqrt(h)); c_a / c_b of the initial diffusion.  float32 values (k int32)."""
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


def euler_schedule(t_start, t_end, dt, N, coeffs):
    """torchsde's fixed-step loop (base_solver.integrate) over ts = linspace(t_start, t_end, 2) in float32: next_t = min(curr_t + dt,
    ts[-1]).  RevVPSDE.f / g evaluate at tt = 1 - curr_t, the start of the step, with the step index kk = long(tt * N)
    (_scale_timesteps); coeffs(tt, kk, step) checks kk and returns that step's (hb, q, gs) as float32 tensors of one element.
    -> the arrays k, h, hb, q, gs of a VPSDESchedule."""
    ts = torch.linspace(t_start, t_end, 2)
    curr, end = ts[0], ts[-1]
    k, h, hb, q, gs = [], [], [], [], []
    while curr < end:
        nxt = min(curr + dt, end)
        tt = 1 - curr.reshape(1)
        kk = int((tt.float() * N).long()[0])
        step = nxt - curr
        hb_t, q_t, gs_t = coeffs(tt, kk, step)
        k.append(kk)
        h.append(float(step))
        hb.append(float(hb_t[0]))
        q.append(float(q_t[0]))
        gs.append(float(gs_t[0]))
        curr = nxt
    return (np.asarray(k, dtype=np.int32),) + tuple(np.asarray(v, dtype=np.float32) for v in (h, hb, q, gs))


class RevVPSDEBase(torch.nn.Module):
    """The part of the reference's RevVPSDE that its two versions share: the discrete and continuous tables, and the time-reversed
    drift f and diffusion g on [B, D] tensors.  A subclass provides vpsde_fn and rvpsde_fn(t, x, return_type)."""

    def __init__(self, model, score_type, beta_min, beta_max, N, model_kwargs):
        super().__init__()
        self.model = model
        self.score_type = score_type
        self.model_kwargs = model_kwargs
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

    def f(self, t, x):
        """The drift -f(x, 1 - t) of the time-reversed SDE (t' = 1 - t), on [B, D]."""
        drift = self.rvpsde_fn(1 - t.expand(x.shape[0]), x, return_type='drift')
        assert drift.shape == x.shape
        return -drift

    def g(self, t, x):
        """The diffusion g(1 - t), broadcast to [B, D]."""
        diffusion = self.rvpsde_fn(1 - t.expand(x.shape[0]), x, return_type='diffusion')
        assert diffusion.shape == (x.shape[0],)
        return diffusion[:, None].expand(x.shape)


def _first_order_only(what):
    if torch.is_grad_enabled():
        raise DmadError("the %s gradient is first-order only: create_graph=True (double backward) is not supported; "
                        "use score_grad='torch' for higher derivatives" % what)


class _ChainNone(torch.autograd.Function):
    """score_grad='none': the inference chain forward; backward = c_a prod(1 + h beta/2) g_out (eps held constant)."""

    @staticmethod
    def forward(ctx, x0, den, sch, sample0):
        ctx.gain = sch.linear_gain()
        return den._run(x0, sch, sample0, path=0).view(x0.shape)

    @staticmethod
    def backward(ctx, g_out):
        _first_order_only("VP-SDE chain's")
        return g_out * ctx.gain, None, None, None


class _ChainHIP(torch.autograd.Function):
    """score_grad='hip' with a gradient: the exact-fp32 chain, its trajectory kept; backward = the purifier's _run_vjp."""

    @staticmethod
    def forward(ctx, x0, den, sch, sample0):
        out, traj = den._run(x0, sch, sample0, path=1, want_traj=True)
        ctx.den, ctx.sch = den, sch
        ctx.save_for_backward(traj)
        return out.view(x0.shape)

    @staticmethod
    def backward(ctx, g_out):
        _first_order_only('HIP VP-SDE')
        traj, = ctx.saved_tensors
        g = ctx.den._run_vjp(traj, ctx.sch, g_out)
        return g.view(g_out.shape).to(g_out.dtype), None, None, None


class ChainPurifier:
    """Mixin of RevDiffWave and RevImprovedDiffusion (see the module docstring for what the class provides)."""
    SCORE_GRADS = ()

    @property
    def score_grad(self) -> str:
        return self._score_grad

    @score_grad.setter
    def score_grad(self, value: str):
        if value not in self.SCORE_GRADS:
            raise ValueError('score_grad must be one of %s, not %r' % (self.SCORE_GRADS, value))
        self._score_grad = value

    @property
    def engine(self):
        return self.model.engine

    def _chain(self, x0, sch):
        sample0 = self._draws
        self._draws += x0.shape[0]
        grad = needs_grad(x0)
        if self._score_grad == 'torch' and grad:
            return self._run_torch(x0, sch, sample0)
        if self._score_grad == 'hip':
            if grad:
                return _ChainHIP.apply(x0, self, sch, sample0)
            with torch.no_grad():                       # the launches of _ChainHIP's forward: the same bits, no trajectory kept
                return self._run(x0, sch, sample0, path=1).view(x0.shape)
        if grad:
            return _ChainNone.apply(x0, self, sch, sample0)
        with torch.no_grad():
            return self._run(x0, sch, sample0, path=0).view(x0.shape)

    def _rounds(self, x0, post=lambda x: x):
        """sample_step rounds of (diffuse to t, reverse VP-SDE chain, post), each round's output the next one's input, the rounds
        concatenated on dim 0.  rand_t moves the diffusion level of a round and keeps its integration range at args.t."""
        xs = []
        for _ in range(self.args.sample_step):
            total_noise_levels = self.args.t
            if self.args.rand_t:
                total_noise_levels = self.args.t + np.random.randint(-self.args.t_delta, self.args.t_delta)
            x0 = post(self._chain(x0, self.schedule(total_noise_levels)))
            xs.append(x0)
        return torch.cat(xs, dim=0)
