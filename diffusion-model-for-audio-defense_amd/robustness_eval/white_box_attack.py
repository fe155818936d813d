"""White-box attack of the adaptive-attack driver: the behaviour of the reference's robustness_eval/white_box_attack.py (stage 1 of
`AudioAttack`, l.276-468, and its norm helpers l.11-36), restated for this package.

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

Differences from the reference: this package's EOT detaches its input, so delta.grad stays None on the EOT gradient path and is only
zeroed when it exists; that EOT averages a per-example loss, so it gets the criterion with reduction='none' (the reference's mean
reduction only scales the gradient by 1/n, which its sign does not see); stage 2 (Qin-I, the psychoacoustic masker, max_iter_2 > 0) is not provided (the reference marks it "not used")
and raises NotImplementedError, as does an unknown norm.  A masker with max_iter_2 = 0 is kept and unused: stage 1 runs, as in the
reference."""
import copy
from typing import Union

import numpy as np
import torch
from torch.nn import CrossEntropyLoss

__all__ = ['AudioAttack', 'lp_norm', 'project_to_norm_ball']

NORMS = ('linf', 'l2')


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


class AudioAttack:
    """The reference's AudioAttack (same arguments and defaults); stage 1 only."""

    def __init__(self, model: torch.nn.Module, masker=None, criterion=CrossEntropyLoss(), eps: float = 2000.0, norm: str = 'linf',
                 learning_rate_1: float = 100.0, max_iter_1: int = 1000, alpha: float = 0.05, learning_rate_2: float = 1.0,
                 max_iter_2: int = 4000, loss_theta_min: float = 0.05, decrease_factor_eps: float = 0.8, num_iter_decrease_eps: int = 10,
                 increase_factor_alpha: float = 1.2, num_iter_increase_alpha: int = 20, decrease_factor_alpha: float = 0.8,
                 num_iter_decrease_alpha: int = 50, eot_attack_size: int = 15, eot_defense_size: int = 15, verbose: int = 1) -> None:
        if norm not in NORMS:
            raise NotImplementedError('Unsupported norm: %s! (%s)' % (norm, ', '.join(NORMS)))
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

    def generate(self, x: Union[torch.Tensor, np.ndarray], y: Union[torch.Tensor, np.ndarray], targeted: bool = True):
        """(x_adv [n, 1, L], (success list of stage 1, None)).  max_iter_2 > 0 (stage 2) raises NotImplementedError; a masker alone does not."""
        if self.max_iter_2 > 0:
            self.stage_2(x, None, y)
        self._targeted = targeted
        if isinstance(x, np.ndarray):
            x = torch.from_numpy(x)
        if isinstance(y, np.ndarray):
            y = torch.from_numpy(y)
        x_adv, success_stage_1 = self.stage_1(x, y)
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

    def stage_2(self, x, x_adv, y=None):
        raise NotImplementedError('AudioAttack stage 2 (Qin-I: the psychoacoustic masker, max_iter_2 > 0) is not provided; the '
                                  'reference marks it "not used" — run stage 1 only (max_iter_2 = 0)')
