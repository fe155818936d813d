"""Host mirror of the reference's diffusion_models/improved_diffusion_sde.py — the reverse VP-SDE purifier on mel spectrograms that the
adaptive-attack driver builds for `--defense Diffusion-Spec` (adaptive_attack_eval.py) — backed by the MI355X engine (libdmad_hip.so).
Same names, constructor signatures and attributes as the reference:

  RevVPSDE(model, score_type='guided_diffusion', beta_min=0.1, beta_max=20, N=1000, img_shape=(1, 32, 32), model_kwargs=None)
      .discrete_betas / .alphas_cumprod / .alphas_cumprod_cont / .sqrt_1m_alphas_cumprod_neg_recip_cont / .noise_type / .sde_type,
      ._scale_timesteps / .vpsde_fn / .rvpsde_fn / .f(t, x) / .g(t, x) on [B, 1024] tensors
  RevImprovedDiffusion(args, config=None, device=None) .model / .diffusion / .rev_vpsde / .betas, .image_editing_sample(img), .forward(x)

Unlike diffwave_sde.py, beta is continuous in t (beta_t = beta_0 + t (beta_1 - beta_0)), the score divides by the
continuous sqrt(1 - abar_c(t)), the noise has no scale factor (every step draws, the last one included), and torchsde runs at its
default dt = 1e-3 because the reference passes none.  `spec_vpsde_schedule` restates that float32 loop on the host; its
UNet step index k = long((1 - curr_t) * 1000) repeats and skips values and reaches 1000 at t = 1000, which is legal here because
nothing is indexed by it.  Each round is then one library call (dmad_spec_vpsde_purify):
x <- c_a x0 + c_b z;  x <- x + (beta/2 x - q eps_k(x)) h + gs z  per step, on the standardised map.

Rounds: the input is melspec_standardize'd once; each of sample_step rounds diffuses its x0, runs the chain and maps the result back
with melspec_inv_standardize, and that mel-dB map is the next round's x0 (as in the reference, it is not standardised again).  The
standardisation stays a torch op around the engine call, so autograd carries its factor.

Noise: on-device Philox keyed (seed, sample0 + row), the first 1024 values of the row (SpecPurifier's convention) — stream 0x5DF00000
for the diffusion draw, 0x5DF00001 + n for Euler step n; row i of a round is sample `_draws + i`, and every round takes the next B
samples.  `use_bm` is accepted and changes nothing: torchsde's Brownian stream is not reproduced.

Gradients (RevImprovedDiffusion(..., score_grad=...)).  The reference calls the UNet outside no_grad, so its adjoint differentiates
through eps: the full gradient is the reference's semantics here.
  'hip'   (default) the forward runs on the exact-fp32 UNet tier with and without a gradient (attack and evaluation forwards are
          bit-identical; with a gradient it also keeps the trajectory, S + 1 maps of 4 kB per spectrogram); the backward is one library
          call (dmad_spec_vpsde_purify_vjp).  FP32 / EXACT engines.
  'torch' the same chain composed from torch ops and UNetModel autograd (the engine's UNet VJP per step) with the same Philox draws —
          the cross-check.
  'none'  eps held constant: the forward runs on the mode's default UNet tier, the backward is c_a * prod(1 + h beta/2) * g_out.
'none' and 'hip' are first-order only: create_graph=True raises DmadError."""
import numpy as np
import torch

from dmad_hip import engine as _eng
from dmad_hip._lib import DmadError
from dmad_hip.autograd import has_unet_vjp
from ._rev_vpsde import ChainPurifier, RevVPSDEBase, VPSDESchedule, _extract_into_tensor, euler_schedule
from .improved_diffusion_ddpm import create_improved_diffusion
from .Improved_Diffusion_Unconditional.improved_diffusion.sc09_spectrogram_dataset import melspec_inv_standardize, melspec_standardize

SPEC_VPSDE_STREAM_DIFFUSE = 0x5DF00000     # Philox stream of the diffusion draw (include/dmad.h dmad_spec_vpsde_purify)
SPEC_VPSDE_STREAM_STEP0 = 0x5DF00001       # ... of Euler step n: SPEC_VPSDE_STREAM_STEP0 + n
SCORE_GRADS = ('hip', 'torch', 'none')
TORCHSDE_DT = 1e-3                         # torchsde.sdeint's default step: the reference passes no dt


def spec_vpsde_schedule(t: int, t_diffuse=None, beta_min=0.1, beta_max=20, N=1000, dt=TORCHSDE_DT) -> VPSDESchedule:
    """The Euler steps of RevImprovedDiffusion.image_editing_sample's sdeint_adjoint(RevVPSDE, ts = linspace(1 - t/1000, 1 - 1e-5, 2),
    'euler') at torchsde's default dt, computed on the host in float32 and in the reference's order.  t_diffuse: the noise level of the
    initial diffusion (c_a, c_b from the discrete linspace(beta_min/N, beta_max/N, N) table); rand_t moves it and keeps the
    integration range at t (default t).  gs = sqrt(beta) sqrt(h): no scale factor, so every step draws."""
    betas = torch.linspace(beta_min / N, beta_max / N, N)
    td = t if t_diffuse is None else int(t_diffuse)
    for name, v in (('t', t), ('t_diffuse', td)):
        if not 1 <= v <= N:
            raise ValueError('%s = %d outside [1, %d]' % (name, v, N))
    a = (1 - betas).cumprod(dim=0)
    c_a, c_b = float(a[td - 1].sqrt()), float((1.0 - a[td - 1]).sqrt())

    def coeffs(tt, kk, step):
        if not 0 <= kk <= N:
            raise ValueError('step index %d outside [0, %d] at t = %d' % (kk, N, t))
        beta_t = beta_min + tt * (beta_max - beta_min)                                      # vpsde_fn
        diffusion = torch.sqrt(beta_t)
        # 1 - alphas_cumprod_cont(tt) as -expm1: 1 - exp(..) loses up to 4 digits in float32 at small tt (1.2e-4 of q at t = 1)
        one_m_abar = -torch.expm1(-0.5 * (beta_max - beta_min) * tt ** 2 - beta_min * tt)
        return 0.5 * beta_t, diffusion ** 2 / torch.sqrt(one_m_abar), diffusion * torch.sqrt(step)
    return VPSDESchedule(*euler_schedule(1 - t * 1. / 1000, 1 - 1e-5, dt, N, coeffs), c_a, c_b)


class RevVPSDE(RevVPSDEBase):
    """The reverse VP-SDE of the reference (drift -f(x, 1 - t), diffusion g(1 - t)) on [B, 1024] tensors, the score from the UNet.
    RevImprovedDiffusion does not integrate it op by op: its chain runs on the engine (spec_vpsde_schedule)."""

    def __init__(self, model, score_type='guided_diffusion', beta_min=0.1, beta_max=20, N=1000, img_shape=(1, 32, 32), model_kwargs=None):
        super().__init__(model, score_type, beta_min, beta_max, N, model_kwargs)
        self.img_shape = img_shape

    def vpsde_fn(self, t, x):
        beta_t = self.beta_0 + t * (self.beta_1 - self.beta_0)
        return -0.5 * beta_t[:, None] * x, torch.sqrt(beta_t)

    def rvpsde_fn(self, t, x, return_type='drift'):
        """Drift (return_type='drift') or diffusion of the reverse SDE at time t (shape [B]).  The UNet runs outside no_grad."""
        drift, diffusion = self.vpsde_fn(t, x)
        if return_type != 'drift':
            return diffusion
        assert x.ndim == 2 and np.prod(self.img_shape) == x.shape[1], x.shape
        if self.score_type != 'guided_diffusion':
            raise NotImplementedError(f'Unknown score type in RevVPSDE: {self.score_type}!')
        eps = self.model(x.view(-1, *self.img_shape), self._scale_timesteps(t), **(self.model_kwargs or {}))
        assert eps.shape == (x.shape[0],) + tuple(self.img_shape), eps.shape
        score = _extract_into_tensor(self.sqrt_1m_alphas_cumprod_neg_recip_cont, t, x.shape) * eps.view(x.shape[0], -1)
        return drift - diffusion[:, None] ** 2 * score


class RevImprovedDiffusion(ChainPurifier, torch.nn.Module):
    """The reference's RevImprovedDiffusion.  Reads args.ddpm_path, t, score_type, sample_step, rand_t, t_delta and use_bm.  Keywords
    beyond the reference's: state_dict / engine (passed to create_improved_diffusion; synthetic weights, an explicit engine),
    score_grad ('hip' | 'torch' | 'none', see the module docstring), seed (Philox key)."""
    SCORE_GRADS = SCORE_GRADS

    def __init__(self, args, config=None, device=None, score_grad='hip', seed=0, state_dict=None, engine=None):
        super().__init__()
        self.args = args
        self.config = config
        if device is None:
            device = torch.device("cuda") if torch.cuda.is_available() else torch.device("cpu")
        self.device = device
        img_shape = (1, 32, 32)
        engine = engine if engine is not None else _eng.get_engine()
        pur = create_improved_diffusion(args.ddpm_path, reverse_timestep=args.t, state_dict=state_dict, engine=engine)
        self.model = pur.model
        self.diffusion = pur.diffusion
        self.rev_vpsde = RevVPSDE(model=self.model, score_type=args.score_type, img_shape=img_shape, model_kwargs=None)
        self.betas = self.rev_vpsde.discrete_betas.float()
        self.score_grad = score_grad
        self.seed = int(seed)
        self._draws = 0
        if score_grad == 'hip' and not has_unet_vjp(self.engine):
            raise DmadError("score_grad='hip' runs the chain on the exact-fp32 UNet tier, which this engine (precision %s) does not hold: "
                            "use an FP32 or EXACT engine, or score_grad='none'" % (self.engine.precision,))

    def schedule(self, t_diffuse=None) -> VPSDESchedule:
        """The Euler steps of one round at args.t (the initial diffusion at t_diffuse, default args.t)."""
        v = self.rev_vpsde
        return spec_vpsde_schedule(self.args.t, t_diffuse=t_diffuse, beta_min=v.beta_0, beta_max=v.beta_1, N=v.N)

    def _run(self, x0, sch, sample0, path, want_traj=False):
        """One chain on the engine, no gradient: [B, 1, 32, 32] standardised -> [B, 32, 32] (and the trajectory)."""
        return self.engine.spec_vpsde_purify(x0, sch.c_a, sch.c_b, sch.k, sch.h, sch.hb, sch.q, sch.gs, seed=self.seed, sample0=sample0,
                                             path=path, want_traj=want_traj)

    def _run_vjp(self, traj, sch, g_out):
        """dmad_spec_vpsde_purify_vjp over the trajectory of _run(.., path=1, want_traj=True); the workspace is reserved on first use."""
        eng, B = self.engine, g_out.shape[0]
        if eng.unet_vjp_batch < min(B, eng.max_batch):
            eng.reserve_unet_vjp(min(B, eng.max_batch))
        return eng.spec_vpsde_purify_vjp(traj, sch.c_a, sch.k, sch.h, sch.hb, sch.q, g_out.reshape(B, 32, 32).contiguous())

    def _noise(self, sample0, stream, B):
        return self.engine.philox_normal(self.seed, sample0, stream, B)[:, :1024].reshape(B, 1, 32, 32)

    def _run_torch(self, x0, sch, sample0):
        """The chain composed from torch ops and UNetModel autograd, with the engine's Philox draws."""
        B = x0.shape[0]
        x = sch.c_a * x0 + sch.c_b * self._noise(sample0, SPEC_VPSDE_STREAM_DIFFUSE, B)
        for n in range(sch.steps):
            eps = self.model(x, torch.full((B,), int(sch.k[n])))
            x = x + (float(sch.hb[n]) * x - float(sch.q[n]) * eps) * float(sch.h[n])
            x = x + float(sch.gs[n]) * self._noise(sample0, SPEC_VPSDE_STREAM_STEP0 + n, B)
        return x

    def image_editing_sample(self, img):
        """Mel-dB spectrograms [B, 1, 32, 32]: standardise, then sample_step rounds of (diffuse to t, reverse VP-SDE chain, map back),
        each round's output the next one's input, the rounds concatenated on dim 0."""
        assert isinstance(img, torch.Tensor)
        assert img.ndim == 4, img.ndim
        if self.rev_vpsde.score_type != 'guided_diffusion':     # the reference raises when sdeint first evaluates the drift
            raise NotImplementedError(f'Unknown score type in RevVPSDE: {self.rev_vpsde.score_type}!')
        x0 = melspec_standardize(img.to(self.device).float())
        return self._rounds(x0, post=melspec_inv_standardize)

    def forward(self, x):
        return self.image_editing_sample(x)
