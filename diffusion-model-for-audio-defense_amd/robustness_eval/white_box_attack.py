"""White-box attacks of the adaptive-attack and imperceptible-attack drivers: the behaviour of the reference's
robustness_eval/white_box_attack.py (`PsychoacousticMasker` l.38-275, `AudioAttack` l.277-728 and the norm helpers l.11-36), restated for
this package.

Stage 1 is a sign-gradient (PGD / "CW" in the driver) loop on a perturbation delta of the waveform:
  * eps and the step size are given in int16 units and scaled by 2**-15 for float32 input;
  * every iteration classifies x + delta (through EOT with `eot_defense_size` > 1), keeps the last successful perturbed clip per
    example, and every `num_iter_decrease_eps` iterations shrinks the bound of the examples that currently succeed to
    min(bound, ||delta||) * decrease_factor_eps;
  * the step follows the sign of the loss gradient (through EOT with `eot_attack_size` > 1), then delta is projected onto the
    linf / l2 ball of its example's bound and x + delta onto the [-1, 1] box;
  * x_adv is the last successful perturbed clip, or the final one; the success list says which.
The gradient flows through whatever the model is: with the HIP backends (CifarResNeXt.grad_backend = 'hip', MelSpectrogramDB(...,
grad_backend='hip'), the SDE purifiers' score_grad='hip') it is computed by the engine's vector-Jacobian products.

Stage 2 (the imperceptible attack of Qin et al. 2019, the driver's `--attack Qin-I`; `max_iter_2` > 0 and a masker) starts from stage 1's
clips and descends  loss_net + alpha * loss_theta,  loss_theta the hinge of the perturbation's normalised power spectral density over
the masking threshold of the clean clip (`PsychoacousticMasker`, once per batch, numpy on the host):
  * every iteration classifies x + delta, keeps per example the successful perturbed clip with the smallest loss_theta so far, every
    `num_iter_increase_alpha` iterations multiplies the alpha of the examples that succeed by `increase_factor_alpha`, every
    `num_iter_decrease_alpha` iterations that of the examples that fail by `decrease_factor_alpha` (not below 0.0005), and steps
    delta <- clamp(x + delta -/+ lr (g_net + alpha g_theta), -1, 1) - x;
  * it stops when every example has once had loss_theta < `loss_theta_min`.
`masking_backend` (new keyword, after the reference's arguments) says where g_theta comes from: 'hip' (default) is one
`Engine.masking_step` call per iteration (dmad_masking_step, DESIGN §20: STFT, hinge, gradient and the update on the engine, in fp32),
with the engine taken from model.classifier; 'torch' is the reference's operators (torch.stft with autograd; the hinge in float64, as
the reference's dtype promotion has it) without its per-iteration copy of delta to the host and back.  Per iteration only the
predictions and the losses of the batch come to the host.  Kept from the reference: it never zeroes delta.grad in stage 2, so g_net is
the SUM of the network gradients of all iterations so far; an exactly-zero STFT bin gives a NaN gradient on the torch branch
(sqrt'(0) * 0) and 0 on the engine.

Differences from the reference: this package's EOT detaches its input, so delta.grad stays None on the EOT gradient path and is only
zeroed when it exists; that EOT averages a per-example loss, so it gets the criterion with reduction='none' (the reference's mean
reduction only scales the gradient by 1/n, which its sign does not see); an unknown norm raises NotImplementedError; `max_iter_2` > 0
with a masker that has no `calculate_threshold_and_psd_maximum` (None, the default) raises NotImplementedError before stage 1, where the
reference would crash after it.  A masker with max_iter_2 = 0 is kept and unused: stage 1 runs, as in the reference.  The masker uses
numpy and scipy only: the reference's librosa.core.stft(center=False) is the framed rfft of the Hann-windowed float32 frames, rounded to
complex64."""
import copy
from typing import Optional, Tuple, Union

import numpy as np
import scipy.signal as ss
import torch
from torch.nn import CrossEntropyLoss

__all__ = ['AudioAttack', 'PsychoacousticMasker', 'lp_norm', 'project_to_norm_ball']

NORMS = ('linf', 'l2')
MASKING_BACKENDS = ('hip', 'torch')
ALPHA_MIN = 0.0005


def project_to_norm_ball(x: torch.Tensor, p: str, eps: float) -> torch.Tensor:
    """x [n, c, L]: clamp to [-eps, eps] (linf), or scale every row whose l2 norm over (c, L) exceeds eps down to eps (l2)."""
    if p == 'linf':
        return torch.clamp(x, -eps, eps)
    if p == 'l2':
        norm = torch.norm(input=x, dim=(1, 2))[:, None, None]
        return x * torch.min(torch.ones_like(norm), eps / norm)
    raise NotImplementedError('Unsupported norm: %s!' % (p,))


def lp_norm(x: torch.Tensor, p: str) -> torch.Tensor:
    """linf: max |x| over everything; l2: the norm over (1, 2) of a 3-d x ([n, 1, 1]) or over dim 1 of a 2-d x ([n])."""
    if p == 'linf':
        return torch.max(torch.abs(x))
    if p == 'l2':
        if x.ndim == 3:
            return torch.norm(input=x, dim=(1, 2))[:, None, None]
        if x.ndim == 2:
            return torch.norm(input=x, dim=(1,))
        raise ValueError('lp_norm(l2) takes a 2-d or 3-d tensor, not %d-d' % x.ndim)
    raise NotImplementedError('Unsupported norm: %s!' % (p,))


def _per_example(criterion):
    """the criterion with reduction='none' (the EOT averages per-example losses)"""
    if getattr(criterion, 'reduction', 'none') != 'none':
        criterion = copy.copy(criterion)
        criterion.reduction = 'none'
    return criterion


def framed_stft(audio: np.ndarray, window_size: int, hop_size: int) -> np.ndarray:
    """librosa.core.stft(audio, n_fft=window_size, hop_length=hop_size, window=hann(fftbins=True), center=False) without librosa: the
    rfft of the windowed frames (float32 samples times the float64 window), rounded to complex64, [window_size // 2 + 1, F] with
    F = (len - window_size) // hop_size + 1."""
    audio = np.asarray(audio, dtype=np.float32)
    if audio.ndim != 1 or audio.shape[0] < window_size:
        raise ValueError('framed_stft takes a 1-d signal of at least %d samples, not %s' % (window_size, audio.shape))
    n_frames = (audio.shape[0] - window_size) // hop_size + 1
    frames = np.lib.stride_tricks.as_strided(audio, shape=(n_frames, window_size), strides=(hop_size * audio.strides[0], audio.strides[0]),
                                             writeable=False)
    window = ss.get_window('hann', window_size, fftbins=True)
    return np.fft.rfft(window[None, :] * frames, axis=1).T.astype(np.complex64)


class PsychoacousticMasker:
    """The psychoacoustic model of Lin and Abdulla (2015) with the simplifications of Qin et al. (2019), as the reference has it
    (l.38-275; same constructor, properties and methods, its quirks included — the module docstring of tests/test_qin_cpu.py lists
    them).  Host only (numpy, scipy): it runs once per batch."""

    def __init__(self, window_size: int = 2048, hop_size: int = 512, sample_rate: int = 16000) -> None:
        self._window_size, self._hop_size, self._sample_rate = window_size, hop_size, sample_rate
        self._fft_frequencies: Optional[np.ndarray] = None
        self._bark: Optional[np.ndarray] = None
        self._absolute_threshold_hearing: Optional[np.ndarray] = None

    def calculate_threshold_and_psd_maximum(self, audio: np.ndarray) -> Tuple[np.ndarray, np.ndarray]:
        """audio [length] -> (global masking threshold in dB [window_size // 2 + 1, F], the maximum of the unnormalised PSD, a scalar)."""
        psd_matrix, psd_max = self.power_spectral_density(audio)
        threshold = np.zeros_like(psd_matrix)
        for frame in range(psd_matrix.shape[1]):
            maskers, masker_idx = self.filter_maskers(*self.find_maskers(psd_matrix[:, frame]))
            threshold[:, frame] = self.calculate_global_threshold(self.calculate_individual_threshold(maskers, masker_idx))
        return threshold, psd_max

    @property
    def window_size(self) -> int:
        return self._window_size

    @property
    def hop_size(self) -> int:
        return self._hop_size

    @property
    def sample_rate(self) -> int:
        return self._sample_rate

    @property
    def fft_frequencies(self) -> np.ndarray:
        if self._fft_frequencies is None:
            self._fft_frequencies = np.linspace(0, self.sample_rate / 2, self.window_size // 2 + 1)
        return self._fft_frequencies

    @property
    def bark(self) -> np.ndarray:
        if self._bark is None:
            f = self.fft_frequencies
            self._bark = 13 * np.arctan(0.00076 * f) + 3.5 * np.arctan(np.square(f / 7500.0))
        return self._bark

    @property
    def absolute_threshold_hearing(self) -> np.ndarray:
        """ATH in dB per bin; -inf outside 20 Hz ... 20 kHz (bins 0 - 2 at the defaults), so a masker there is never filtered."""
        if self._absolute_threshold_hearing is None:
            valid = np.logical_and(20 <= self.fft_frequencies, self.fft_frequencies <= 2e4)
            khz = self.fft_frequencies[valid] * 0.001
            ath = np.ones(valid.shape) * -np.inf
            ath[valid] = 3.64 * pow(khz, -0.8) - 6.5 * np.exp(-0.6 * np.square(khz - 3.3)) + 0.001 * pow(khz, 4) - 12
            self._absolute_threshold_hearing = ath
        return self._absolute_threshold_hearing

    def power_spectral_density(self, audio: np.ndarray) -> Tuple[np.ndarray, np.ndarray]:
        """audio [length] -> (PSD in dB normalised to a maximum of 96 [window_size // 2 + 1, F], the maximum before normalisation)."""
        stft_matrix = framed_stft(audio.astype(np.float32), self.window_size, self.hop_size)
        with np.errstate(divide='ignore'):
            gain_factor = np.sqrt(8.0 / 3.0)
            psd_matrix = 20 * np.log10(np.abs(gain_factor * stft_matrix / self.window_size))
            psd_matrix = psd_matrix.clip(min=-200)
        psd_matrix_max = np.max(psd_matrix)
        return 96.0 - psd_matrix_max + psd_matrix, psd_matrix_max

    @staticmethod
    def find_maskers(psd_vector: np.ndarray) -> Tuple[np.ndarray, np.ndarray]:
        """The strict local maxima of one frame (edges never), each smoothed with its two neighbours in the power domain; all tonal."""
        masker_idx = ss.argrelmax(psd_vector)[0]
        power = 10 ** (psd_vector[masker_idx - 1] / 10) + 10 ** (psd_vector[masker_idx] / 10) + 10 ** (psd_vector[masker_idx + 1] / 10)
        return 10 * np.log10(power), masker_idx

    def filter_maskers(self, maskers: np.ndarray, masker_idx: np.ndarray) -> Tuple[np.ndarray, np.ndarray]:
        """Drops the maskers at or below the ATH, then the smaller of two maskers closer than 0.5 bark.  The reference's bark loop is kept
        as it is: it reads self.bark at the POSITION in the masker list (i, i_prev), not at the masker's bin, and moves i_prev to
        i_prev + 1 (not to i) when it drops the earlier masker."""
        keep = maskers > self.absolute_threshold_hearing[masker_idx]
        masker_idx, maskers = masker_idx[keep], maskers[keep]
        keep = np.ones(masker_idx.shape, dtype=bool)
        i_prev = 0
        for i in range(1, len(masker_idx)):
            if self.bark[i] - self.bark[i_prev] < 0.5:
                if maskers[i_prev] < maskers[i]:
                    keep[i_prev] = False
                    i_prev = i_prev + 1
                else:
                    keep[i] = False
            else:
                i_prev = i
        return maskers[keep], masker_idx[keep]

    def calculate_individual_threshold(self, maskers: np.ndarray, masker_idx: np.ndarray) -> np.ndarray:
        """[maskers, window_size // 2 + 1]: masker + delta_shift[its bin] + the two-slope spread function over the bark distance."""
        delta_shift = -6.025 - 0.275 * self.bark
        threshold = np.zeros(masker_idx.shape + self.bark.shape)
        for k, (masker_j, masker) in enumerate(zip(masker_idx, maskers)):
            delta_z = self.bark - self.bark[masker_j]
            spread = 27 * delta_z
            up = delta_z > 0
            spread[up] = (-27 + 0.37 * max(masker - 40, 0)) * delta_z[up]
            threshold[k, :] = masker + delta_shift[masker_j] + spread
        return threshold

    def calculate_global_threshold(self, individual_threshold: np.ndarray) -> np.ndarray:
        """10 log10(sum over the maskers of 10^(T / 10) + 10^(ATH / 10)) per bin"""
        with np.errstate(divide='ignore'):
            return 10 * np.log10(np.sum(10 ** (individual_threshold / 10), axis=0) + 10 ** (self.absolute_threshold_hearing / 10))


class AudioAttack:
    """The reference's AudioAttack (same arguments and defaults, then `masking_backend`): stage 1 and, with a masker and max_iter_2 > 0,
    stage 2.  `trace` (None, or a list set by a test or a tool) receives one dict per stage-2 iteration: 'prediction', 'alpha' and
    'loss_theta' as lists per example."""

    def __init__(self, model: torch.nn.Module, masker=None, criterion=CrossEntropyLoss(), eps: float = 2000.0, norm: str = 'linf',
                 learning_rate_1: float = 100.0, max_iter_1: int = 1000, alpha: float = 0.05, learning_rate_2: float = 1.0,
                 max_iter_2: int = 4000, loss_theta_min: float = 0.05, decrease_factor_eps: float = 0.8, num_iter_decrease_eps: int = 10,
                 increase_factor_alpha: float = 1.2, num_iter_increase_alpha: int = 20, decrease_factor_alpha: float = 0.8,
                 num_iter_decrease_alpha: int = 50, eot_attack_size: int = 15, eot_defense_size: int = 15, verbose: int = 1,
                 masking_backend: str = 'hip') -> None:
        if norm not in NORMS:
            raise NotImplementedError('Unsupported norm: %s! (%s)' % (norm, ', '.join(NORMS)))
        if masking_backend not in MASKING_BACKENDS:
            raise ValueError('masking_backend must be one of %s, not %r' % (MASKING_BACKENDS, masking_backend))
        self.masking_backend = masking_backend
        self.trace = None
        self.model, self.masker, self.criterion = model, masker, criterion
        self.eps, self.norm = eps, norm
        self.learning_rate_1, self.max_iter_1 = learning_rate_1, max_iter_1
        self.alpha, self.learning_rate_2, self.max_iter_2 = alpha, learning_rate_2, max_iter_2
        self._targeted = True
        self.loss_theta_min = loss_theta_min
        self.decrease_factor_eps, self.num_iter_decrease_eps = decrease_factor_eps, num_iter_decrease_eps
        self.increase_factor_alpha, self.num_iter_increase_alpha = increase_factor_alpha, num_iter_increase_alpha
        self.decrease_factor_alpha, self.num_iter_decrease_alpha = decrease_factor_alpha, num_iter_decrease_alpha
        self.scale_factor = 2 ** -15
        self.eot_attack_size, self.eot_defense_size = eot_attack_size, eot_defense_size
        self.verbose = verbose
        if self.eot_attack_size > 1 or self.eot_defense_size > 1:
            from ._EOT import EOT
            self.eot_model = EOT(model=model, loss=_per_example(self.criterion), EOT_size=eot_attack_size)
        if self._has_masker():
            self._window_size, self._hop_size, self._sample_rate = masker.window_size, masker.hop_size, masker.sample_rate

    def _has_masker(self):
        return hasattr(self.masker, 'calculate_threshold_and_psd_maximum')

    def _find_engine(self, x):
        """the engine of masking_backend='hip': the one bound to model.classifier; refuses a CPU input"""
        from dmad_hip._lib import DmadError
        engine = getattr(getattr(self.model, 'classifier', None), '__dict__', {}).get('engine')
        if engine is None:
            raise DmadError("AudioAttack(masking_backend='hip') needs an engine: none is bound to model.classifier (the dmad engine has "
                            "no CPU path; masking_backend='torch' runs anywhere)")
        if not x.is_cuda:
            raise DmadError("AudioAttack(masking_backend='hip'): input must live on the GPU (the dmad engine has no CPU path; "
                            "masking_backend='torch' runs anywhere)")
        if (self._window_size, self._hop_size) != (2048, 512):
            raise DmadError("AudioAttack(masking_backend='hip') serves the masker's default window 2048 / hop 512 only")
        return engine

    def generate(self, x: Union[torch.Tensor, np.ndarray], y: Union[torch.Tensor, np.ndarray], targeted: bool = True):
        """(x_adv [n, 1, L], (success list of stage 1, success list of stage 2 or None)).  Stage 2 runs with max_iter_2 > 0 and a masker;
        max_iter_2 > 0 without one raises NotImplementedError before stage 1; a masker alone (max_iter_2 = 0) does not."""
        if self.max_iter_2 > 0 and not self._has_masker():
            raise NotImplementedError('AudioAttack stage 2 (Qin-I, max_iter_2 > 0) needs a masker with calculate_threshold_and_psd_maximum '
                                      '(PsychoacousticMasker()); run stage 1 only with max_iter_2 = 0')
        self._targeted = targeted
        if isinstance(x, np.ndarray):
            x = torch.from_numpy(x)
        if isinstance(y, np.ndarray):
            y = torch.from_numpy(y)
        if self.max_iter_2 > 0 and self.masking_backend == 'hip':
            self._find_engine(x)                # refuse before stage 1's work
        x_adv, success_stage_1 = self.stage_1(x, y)
        if self.max_iter_2 > 0:
            x_adv, success_stage_2 = self.stage_2(x, x_adv, y)
            return x_adv, (success_stage_1, success_stage_2)
        return x_adv, (success_stage_1, None)

    def _hits(self, prediction, y):
        """per example: the attack currently succeeds (targeted: predicted == y, untargeted: predicted != y)."""
        same = (prediction.view(-1) == y.view(-1)).tolist()
        return [s if self._targeted else not s for s in same]

    def stage_1(self, x: torch.Tensor, y: torch.Tensor):
        """x: waveforms [n, 1, L]; y: the target labels (targeted) or the true labels (untargeted)."""
        if x.dtype == torch.float32:
            eps, lr = self.scale_factor * self.eps, self.scale_factor * self.learning_rate_1
        else:
            eps, lr = self.eps, self.learning_rate_1
        n = x.shape[0]
        x_adv = [None] * n
        delta = torch.zeros_like(x, requires_grad=True)
        epsilon = [eps] * n
        for i in range(self.max_iter_1 + 1):
            x_pert = x + delta
            if self.eot_defense_size > 1:
                self.eot_model.EOT_size = self.eot_defense_size
                self.eot_model.use_grad = False
                y_pert = self.eot_model(x_pert, y)[0]
            else:
                y_pert = self.model(x_pert)
            hits = self._hits(y_pert.max(1, keepdim=True)[1], y)
            for j in range(n):                  # the last successful perturbed clip (a clean miss counts as one)
                if hits[j]:
                    x_adv[j] = x_pert[j].detach()
            if i % self.num_iter_decrease_eps == 0 and i > 0:
                for j in range(n):
                    if hits[j]:
                        norm = lp_norm(delta.data[j], p=self.norm).item()
                        if epsilon[j] > norm:
                            epsilon[j] = norm
                        epsilon[j] *= self.decrease_factor_eps
            if i == self.max_iter_1:
                break
            if self.eot_attack_size > 1:
                self.eot_model.EOT_size = self.eot_attack_size
                self.eot_model.use_grad = True
                grad = self.eot_model(x_pert, y)[2]
            else:
                loss = self.criterion(y_pert, y)
                loss.backward()
                grad = delta.grad
            step = lr * grad.data.sign()
            delta.data = delta.data - step if self._targeted else delta.data + step
            delta.data = torch.cat([project_to_norm_ball(torch.unsqueeze(p, 1), self.norm, e) for p, e in zip(delta.data, epsilon)], dim=0)
            delta.data = (x + delta.data).clamp(-1, 1) - x
            if delta.grad is not None:
                delta.grad.zero_()
        x_pert = (x + delta).detach()
        success_stage_1 = [True] * n
        for j in range(n):                      # no adversarial example found: the final perturbed clip
            if x_adv[j] is None:
                if self.verbose:
                    print('Adversarial attack stage 1 for x_{} was not successful'.format(j))
                x_adv[j] = x_pert[j]
                success_stage_1[j] = False
        return torch.unsqueeze(torch.cat(x_adv, dim=0), 1), success_stage_1

    def stage_2(self, x: torch.Tensor, x_adv: torch.Tensor, y: torch.Tensor = None):
        """x: the clean waveforms [n, 1, L]; x_adv: stage 1's result; y as in stage 1 -> (x_imperceptible [n, 1, L], success list)."""
        if not self._has_masker():
            raise NotImplementedError('AudioAttack stage 2 needs a masker with calculate_threshold_and_psd_maximum (PsychoacousticMasker())')
        lr = self.scale_factor * self.learning_rate_2 if x.dtype == torch.float32 else self.learning_rate_2
        hip = self.masking_backend == 'hip'
        engine = self._find_engine(x) if hip else None
        n = x.shape[0]
        early_stop = [False] * n
        alpha = torch.tensor([self.alpha] * n, dtype=torch.float32).to(x.device)[:, None, None]
        loss_theta_previous = [float('inf')] * n
        loss_theta = [float('inf')] * n
        x_imperceptible = [None] * n
        theta, psd_maximum = self._stabilized_threshold_and_psd_maximum(x)
        if hip:
            theta32, psd_scale = theta.float(), (pow(10.0, 9.6) / psd_maximum).float()
        delta = torch.zeros_like(x, requires_grad=True)
        delta.data = (x_adv.data - x.data).contiguous()
        for i in range(self.max_iter_2 + 1):
            x_pert = x + delta
            y_adv = self.model(x_pert)
            prediction = y_adv.max(1, keepdim=True)[1]
            hits = self._hits(prediction, y)
            for j in range(n):                  # the successful perturbed clip with the smallest masking loss so far
                if hits[j] and loss_theta[j] < loss_theta_previous[j]:
                    x_imperceptible[j] = x_pert[j].detach()
                    loss_theta_previous[j] = loss_theta[j]
            if i > 0 and (i % self.num_iter_increase_alpha == 0 or i % self.num_iter_decrease_alpha == 0):
                hit = torch.tensor(hits, device=x.device)[:, None, None]
                if i % self.num_iter_increase_alpha == 0:
                    alpha = torch.where(hit, alpha * self.increase_factor_alpha, alpha)
                if i % self.num_iter_decrease_alpha == 0:
                    alpha = torch.where(hit, alpha, (alpha * self.decrease_factor_alpha).clamp(min=ALPHA_MIN))
            if i == self.max_iter_2:
                break
            loss = self.criterion(y_adv, y)
            loss.backward()
            g_net = delta.grad.data             # never zeroed, as in the reference: the sum over the iterations so far
            signed_lr = -lr if self._targeted else lr
            if hip:                             # STFT, hinge, gradient and the update in one engine call
                loss_theta = engine.masking_step(x, delta.data, g_net, alpha, signed_lr, theta32, psd_scale).tolist()
            else:
                g_theta, loss_t = self._loss_gradient_masking_threshold(delta, x, theta, psd_maximum)
                assert g_net.shape == g_theta.shape
                delta.data = delta.data + signed_lr * (g_net + alpha * g_theta)
                delta.data = (x + delta.data).clamp(-1, 1) - x
                loss_theta = loss_t.tolist()
            if self.trace is not None:
                self.trace.append({'prediction': prediction.view(-1).tolist(), 'alpha': alpha.view(-1).tolist(), 'loss_theta': list(loss_theta)})
            for j in range(n):
                if loss_theta[j] < self.loss_theta_min and not early_stop[j]:
                    if self.verbose:
                        print('Batch sample {} reached minimum threshold of {} for theta loss.'.format(j, self.loss_theta_min))
                    early_stop[j] = True
            if all(early_stop):
                if self.verbose:
                    print('All batch samples reached minimum threshold for theta loss. Stopping early at iteration {}'.format(i))
                break
        success_stage_2 = [True] * n
        x_pert = x_pert.detach()
        for j in range(n):                      # no imperceptible adversarial example found: the last perturbed clip classified
            if x_imperceptible[j] is None:
                if self.verbose:
                    print('Adversarial attack stage 2 for x_{} was not successful'.format(j))
                x_imperceptible[j] = x_pert[j]
                success_stage_2[j] = False
        return torch.unsqueeze(torch.cat(x_imperceptible, dim=0), 1), success_stage_2

    def _loss_gradient_masking_threshold(self, perturbation: torch.Tensor, x: torch.Tensor, masking_threshold_stabilized: torch.Tensor,
                                         psd_maximum_stabilized: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
        """(d sum(loss) / d perturbation [n, 1, L], loss [n]) of the hinge mean(relu(psd(perturbation) - threshold)) per example.
        'torch': the reference's operators on the device of x (no copy to the host); 'hip': dmad_masking_loss_vjp."""
        p = perturbation.detach()
        p = p[:, 0] if p.ndim == 3 else p
        if self.masking_backend == 'hip':
            g, loss = self._find_engine(x).masking_loss_vjp(p, masking_threshold_stabilized.float(),
                                                            (pow(10.0, 9.6) / psd_maximum_stabilized).float())
            return g.unsqueeze(1), loss
        p = p.clone().requires_grad_(True)
        psd = self._approximate_power_spectral_density(p, psd_maximum_stabilized)
        loss = torch.mean(torch.nn.ReLU()(psd - masking_threshold_stabilized), dim=(1, 2), keepdims=False)
        loss.sum().backward()
        return p.grad.detach().unsqueeze(1), loss.detach()

    def _approximate_power_spectral_density(self, perturbation: torch.Tensor, psd_maximum_stabilized: torch.Tensor) -> torch.Tensor:
        """perturbation [n, L] -> 10^9.6 / psd_max |sqrt(8/3) stft / window|^2 [n, window // 2 + 1, F]: the normalised PSD with the
        10 log10 cancelled (float64 where psd_maximum_stabilized is, as in the reference)."""
        stft = torch.view_as_real(torch.stft(perturbation, n_fft=self._window_size, hop_length=self._hop_size, win_length=self._window_size,
                                             center=False, window=torch.hann_window(self._window_size).to(perturbation.device),
                                             return_complex=True))
        gain_factor = float(np.sqrt(8.0 / 3.0))
        stft_abs = torch.sqrt(torch.sum(torch.square(gain_factor * stft / self._window_size), -1))
        return pow(10.0, 9.6) / psd_maximum_stabilized.reshape(-1, 1, 1) * torch.square(stft_abs)

    def _stabilized_threshold_and_psd_maximum(self, x: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
        """x [n, 1, L] -> (10^(threshold / 10) [n, window // 2 + 1, F], 10^(psd_max / 10) [n]) of the masker, float64 on x's device"""
        xs = x.detach().cpu().numpy()
        xs = xs[:, 0] if xs.ndim > 2 else xs
        pairs = [self.masker.calculate_threshold_and_psd_maximum(x_i) for x_i in xs]
        theta = 10 ** (np.array([t for t, _ in pairs]) * 0.1)
        psd_maximum = 10 ** (np.array([m for _, m in pairs]) * 0.1)
        return torch.from_numpy(theta).to(x.device), torch.from_numpy(psd_maximum).to(x.device)
