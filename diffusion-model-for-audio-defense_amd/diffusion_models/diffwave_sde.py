"""Host mirror of the reference's diffusion_models/diffwave_sde.py — the reverse VP-SDE DiffWave purifier that the adaptive-attack
driver builds for `--defense Diffusion` (adaptive_attack_eval.py) — backed by the MI355X engine (libdmad_hip.so).  Same names,
constructor signatures and attributes as the reference:

  RevVPSDE(model, score_type='ddpm', beta_min=0.02, beta_max=4, N=200, audio_shape=(1, 16000), model_kwargs=None)
      .discrete_betas / .alphas_cumprod / .sqrt_1m_alphas_cumprod / .noise_type / .sde_type,
      ._scale_timesteps / .vpsde_fn / .rvpsde_fn / .f(t, x) / .g(t, x) on [B, L] tensors
  RevDiffWave(args, device=None) .T / .model / .rev_vpsde / .betas, .audio_editing_sample(audio), .forward(x)

The reference integrates the reverse SDE with torchsde.sdeint_adjoint (Euler, dt = 1/T).  torchsde is not used here: at a fixed
step its loop is a short chain, and this project owns it (_rev_vpsde.py, shared with improved_diffusion_sde.py).  `vpsde_schedule`
restates that loop in float32 and in torchsde's order, which repeats and skips step indices; the
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
import numpy as np
import torch

from dmad_hip import autograd as _ag
from dmad_hip import engine as _eng
from dmad_hip._lib import DmadError
from ._rev_vpsde import ChainPurifier, RevVPSDEBase, VPSDESchedule, _extract_into_tensor, euler_schedule  # noqa: F401  (reference export)
from .diffwave_ddpm import DiffWave, create_diffwave_model, fixed_length_only

VPSDE_STREAM_DIFFUSE = 0x5DE00000          # Philox stream of the diffusion draw (include/dmad.h dmad_vpsde_purify)
VPSDE_STREAM_STEP0 = 0x5DE00001            # ... of Euler step n: VPSDE_STREAM_STEP0 + n
SCORE_GRADS = ('none', 'hip', 'torch')


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

    def coeffs(tt, kk, step):
        if not 0 <= kk < N:
            raise ValueError('step index %d outside [0, %d) at t = %d' % (kk, N, t))
        beta_t = beta_0 + (tt * N - 1) / (N - 1) * (beta_1 - beta_0)          # vpsde_fn
        diffusion = torch.sqrt(beta_t)
        scale = torch.sqrt(1 - alphas_cumprod[kk - 1]) / torch.sqrt(1 - alphas_cumprod[kk]) if kk > 0 else torch.zeros(())
        return 0.5 * beta_t, diffusion ** 2 / sqrt_1m[kk], scale * diffusion * torch.sqrt(step)
    return VPSDESchedule(*euler_schedule(1 - t / T, 1 - 1e-5, 1. / T, N, coeffs), c_a, c_b)


class RevVPSDE(RevVPSDEBase):
    """The reverse VP-SDE of the reference (drift -f(x, 1 - t), diffusion g(1 - t)) on [B, L] tensors, with the score from the DiffWave
    mirror's eps-network.  RevDiffWave does not integrate it op by op: its chain runs on the engine (vpsde_schedule)."""

    def __init__(self, model: DiffWave, score_type='ddpm', beta_min=0.02, beta_max=4, N=200, audio_shape=(1, 16000), model_kwargs=None):
        super().__init__(model, score_type, beta_min, beta_max, N, model_kwargs)
        self.audio_shape = audio_shape

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


class RevDiffWave(ChainPurifier, torch.nn.Module):
    """The reference's RevDiffWave (explicitly adapted for DiffWave).  Reads args.ddpm_path, ddpm_config, t, score_type, sample_step,
    rand_t, t_delta and use_bm.  Keywords beyond the reference's: state_dict / engine / precision / max_batch / grad_backend / any_length
    (passed to create_diffwave_model; synthetic weights; any_length serves `.model`, the DDPM DiffWave: the VP-SDE chain of forward() runs
    at the engine's clip_len only), score_grad ('none' | 'hip' | 'torch', see the module docstring), seed (Philox key)."""
    SCORE_GRADS = SCORE_GRADS

    def __init__(self, args, device=None, score_grad='none', seed=0, **kw):
        super().__init__()
        self.args = args
        if device is None:
            device = torch.device("cuda") if torch.cuda.is_available() else torch.device("cpu")
        self.device = device
        audio_shape = (1, 16000)
        extra = {key: kw.pop(key) for key in ('state_dict', 'engine', 'precision', 'max_batch', 'grad_backend', 'any_length') if key in kw}
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

    def schedule(self, t_diffuse=None) -> VPSDESchedule:
        """The Euler steps of one round at args.t (the initial diffusion at t_diffuse, default args.t)."""
        return vpsde_schedule(self.args.t, self.T, self.T, self.rev_vpsde.discrete_betas, self.rev_vpsde.beta_0, self.rev_vpsde.beta_1,
                              t_diffuse=t_diffuse)

    def _run(self, x0, sch, sample0, path, want_traj=False):
        """One chain on the engine, no gradient: [B, 1, L] -> [B, L] (and the trajectory)."""
        return self.engine.vpsde_purify(x0, sch.c_a, sch.c_b, sch.k, sch.h, sch.hb, sch.q, sch.gs, seed=self.seed, sample0=sample0, path=path,
                                        want_traj=want_traj)

    def _run_vjp(self, traj, sch, g_out):
        """dmad_vpsde_purify_vjp over the trajectory of _run(.., path=1, want_traj=True); the VJP workspace is reserved on first use."""
        eng, B = self.engine, g_out.shape[0]
        if eng.vjp_batch < min(B, eng.max_batch):
            eng.reserve_vjp(min(B, eng.max_batch))
        return eng.vpsde_purify_vjp(traj, sch.c_a, sch.k, sch.h, sch.hb, sch.q, g_out.reshape(B, -1).contiguous())

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

    def audio_editing_sample(self, audio):
        """audio in [-1, 1], [B, 1, L]: sample_step rounds of (diffuse to t, reverse VP-SDE chain), each round's output the next one's
        input, the rounds concatenated on dim 0."""
        assert isinstance(audio, torch.Tensor)
        assert audio.ndim == 3, audio.ndim
        fixed_length_only(self.model.model, audio, 'the reverse VP-SDE chain (RevDiffWave.forward)')
        x0 = audio.to(self.device)
        if self.rev_vpsde.score_type != 'guided_diffusion':     # the reference raises when sdeint first evaluates the drift
            raise NotImplementedError(f'Unknown score type in RevVPSDE: {self.rev_vpsde.score_type}!')
        return self._rounds(x0)

    def forward(self, x):
        return self.audio_editing_sample(x)
