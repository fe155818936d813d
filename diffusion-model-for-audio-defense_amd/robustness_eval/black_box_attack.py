"""Query-only attack of the black-box driver: the behaviour of the reference's robustness_eval/black_box_attack.py `FAKEBOB`
(l.13-219; "Who is real Bob? Adversarial Attacks on Speaker Recognition Systems", IEEE S&P 2021), restated for this package.

FAKEBOB is a sign-gradient loop on the waveform whose gradient is the NES estimate (`_NES.NES`) of the per-example loss under the EOT
wrapper (`_EOT.EOT`), with momentum, a per-clip step size that is cut when the loss plateaus, and a convergence test every
`stop_early_iter` iterations that takes clips out of the working batch:
  * every iteration: one NES call on the working batch -> the mean probe loss, the gradient estimate, and the loss / majority decision
    of the unperturbed clip; `success` and the best clip are updated from that unperturbed probe;
  * grad <- momentum * prev_grad + (1 - momentum) * grad;  x <- clip(x + grad_sign * lr * sign(grad), x0 - epsilon, x0 + epsilon) and
    into [-1, 1];
  * the last `plateau_length` mean probe losses of a clip: when the newest exceeds the oldest, lr <- max(lr / plateau_drop, min_lr) and
    the history restarts.

`noise_source` / `seed` / `engine` are passed to NES: with noise_source='device' the probe directions are Philox draws made and consumed
on the engine instead of torch.randn tensors; the default 'torch' consumes torch's generator in the reference's order.
The estimator is built at the first generate() and kept (the reference builds an identical, stateless one per gradient): its draw
counter runs on from batch to batch and from call to call, so one attacker never uses a probe key twice.  `engine` is what lets a model
that is a plain callable (no AcousticSystem around an engine-bound classifier) use the device draws.

The reference's quirks are part of the contract (tests/golden/fakebob.npz is recorded from the reference and judges all of them):
  * the per-clip loss histories start as ONE list shared by all clips (`[[]] * n`), so in the first iteration clip j's history also
    holds the losses of the clips before it; every entry becomes a list of its own as soon as it is first trimmed;
  * the only task with a loss is 'SCR', and that loss is unreduced cross-entropy, which is never negative: the removal of "found" clips
    on the unperturbed loss never removes one.  Only the convergence test does, and it removes a clip whose mean probe loss did not FALL
    by 0.01 % since the last test, whichever way the attack moves the loss;
  * after a convergence test has removed clips, the remembered losses keep the length and order of the batch BEFORE the removal, so the
    next test compares a surviving clip with the loss remembered at its new position;
  * the best clip is the one with the SMALLEST loss of the unperturbed probe, for an untargeted attack too;
  * `success` is set from the majority decision of the unperturbed probe, at any iteration, and is never cleared.
`estimate_threshold` / `estimate_threshold_run` (l.221-311) serve speaker verification, a task this package has no loss for: they raise
NotImplementedError, as does generate() for task 'SV' / 'OSI' without a threshold.  SirenAttack and Kenansville are not provided.
"""
import numpy as np
import torch

from ._EOT import EOT
from ._NES import NES
from ._utils import resolve_loss

__all__ = ['FAKEBOB']


class FAKEBOB:

    def __init__(self, model, threshold=None, task='CSI', targeted=False, confidence=0.5, epsilon=0.002, max_iter=200, max_lr=0.001,
                 min_lr=1e-6, samples_per_draw=50, samples_per_draw_batch_size=50, sigma=0.001, momentum=0.9, plateau_length=5,
                 plateau_drop=2., stop_early=True, stop_early_iter=100, batch_size=1, EOT_size=1, EOT_batch_size=1, verbose=1,
                 noise_source='torch', seed=0, engine=None):
        self.model = model
        self.threshold = threshold
        self.task = task
        self.targeted = targeted
        self.confidence = confidence
        self.epsilon = epsilon
        self.max_iter = max_iter
        self.max_lr = max_lr
        self.min_lr = min_lr
        self.samples_per_draw = samples_per_draw
        self.samples_per_draw_batch_size = samples_per_draw_batch_size
        self.sigma = sigma
        self.momentum = momentum
        self.plateau_length = plateau_length
        self.plateau_drop = plateau_drop
        self.stop_early = stop_early
        self.stop_early_iter = stop_early_iter
        self.batch_size = batch_size
        self.EOT_size = EOT_size
        self.EOT_batch_size = EOT_batch_size
        self.verbose = verbose
        self.noise_source = noise_source
        self.seed = seed
        self.engine = engine
        self.NES_wrapper = None                    # built by the first generate(), then kept: see the module docstring

    # ---------------------------------------------------------------------------------------------------------------- one batch
    def attack_batch(self, x_batch, y_batch, lower, upper, batch_id):
        with torch.no_grad():
            n_audios = x_batch.shape[0]
            last_ls = [[]] * n_audios                       # ONE history, n references to it (see the module docstring)
            lr = [self.max_lr] * n_audios
            prev_loss = [np.inf] * n_audios
            adver_x = x_batch.clone()
            grad = torch.zeros_like(x_batch)
            best_adver_x = adver_x.clone()
            best_loss = [np.inf] * n_audios
            consider_index = list(range(n_audios))       # position in the working batch -> clip of x_batch
            success = [False] * n_audios

            for it in range(self.max_iter + 1):
                prev_grad = grad.clone()
                loss, grad, adver_loss, _, y_pred = self.get_grad(adver_x, y_batch)
                for ii, adver_l in enumerate(adver_loss):
                    index = consider_index[ii]
                    if bool(y_pred[ii] == y_batch[ii]) == bool(self.targeted):
                        success[index] = True
                    if adver_l < best_loss[index]:
                        best_loss[index] = adver_l.cpu().item()
                        best_adver_x[index] = adver_x[ii]
                if self.verbose:
                    print("batch: {} iter: {}, loss: {}, y: {}, y_pred: {}, best loss: {}".format(
                        batch_id, it, adver_loss.cpu().numpy(), y_batch.cpu().numpy(), y_pred, best_loss))

                # clips whose unperturbed loss went negative are done (never, with cross-entropy)
                state = self.delete_found(adver_loss, adver_x, y_batch, prev_grad, grad, lower, upper, consider_index, last_ls, lr,
                                          prev_loss, loss)
                adver_x, y_batch, prev_grad, grad, lower, upper, consider_index, last_ls, lr, prev_loss, loss = state
                if adver_x is None:
                    break
                if it == self.max_iter:
                    continue

                grad = self.momentum * prev_grad + (1.0 - self.momentum) * grad
                for jj, loss_ in enumerate(loss):
                    last_ls[jj].append(loss_)
                    last_ls[jj] = last_ls[jj][-self.plateau_length:]
                    if last_ls[jj][-1] > last_ls[jj][0] and len(last_ls[jj]) == self.plateau_length:
                        if lr[jj] > self.min_lr:
                            lr[jj] = max(lr[jj] / self.plateau_drop, self.min_lr)
                        last_ls[jj] = []
                lr_t = torch.tensor(lr, device=adver_x.device, dtype=torch.float).unsqueeze(1).unsqueeze(2)
                adver_x = adver_x + self.grad_sign * lr_t * torch.sign(grad)
                adver_x = torch.min(torch.max(adver_x, lower), upper)

                if self.stop_early and it % self.stop_early_iter == 0:
                    loss_np = torch.stack(list(loss)).cpu().numpy()
                    converge_loss = np.array(prev_loss) * 0.9999 - loss_np
                    state = self.delete_found(converge_loss, adver_x, y_batch, prev_grad, grad, lower, upper, consider_index, last_ls, lr,
                                              prev_loss, loss)
                    adver_x, y_batch, prev_grad, grad, lower, upper, consider_index, last_ls, lr, prev_loss, loss = state
                    if adver_x is None:
                        break
                    prev_loss = loss_np                       # of the batch BEFORE the removal (see the module docstring)
            return best_adver_x, success

    def delete_found(self, adver_loss, adver_x, y_batch, prev_grad, grad, lower, upper, consider_index, last_ls, lr, prev_loss, loss):
        """Keeps the positions whose `adver_loss` is not negative: the tensors sliced, the lists filtered; (None, ..., []) when none is left."""
        keep = [ii for ii, adver_l in enumerate(adver_loss) if not adver_l < 0]
        if not keep:
            return None, None, None, None, None, None, [], [], [], [], []
        rows = torch.as_tensor(keep, device=adver_x.device)
        pick = lambda t: t.index_select(0, rows)
        take = lambda seq: [seq[ii] for ii in keep]
        return (pick(adver_x), pick(y_batch), pick(prev_grad), pick(grad), pick(lower), pick(upper), take(consider_index), take(last_ls),
                take(lr), take(prev_loss), take(loss))

    def get_grad(self, x, y):
        return self.NES_wrapper(x, y)

    # ---------------------------------------------------------------------------------------------------------------- all clips
    def generate(self, x, y, targeted=False):
        if self.task in ('SV', 'OSI') and self.threshold is None:
            raise NotImplementedError('FAKEBOB for task %s needs a decision threshold, and estimating one (estimate_threshold) is speaker '
                                      'verification, which this package has no loss for' % (self.task,))
        self.targeted = targeted
        self.loss, self.grad_sign = resolve_loss('Margin', self.targeted, self.confidence, self.task, self.threshold, False)
        self.EOT_wrapper = EOT(self.model, self.loss, self.EOT_size, self.EOT_batch_size, False)
        if self.NES_wrapper is None:
            self.NES_wrapper = NES(self.samples_per_draw, self.samples_per_draw_batch_size, self.sigma, self.EOT_wrapper,
                                   noise_source=self.noise_source, seed=self.seed, engine=self.engine)
        else:
            self.NES_wrapper.EOT_wrapper = self.EOT_wrapper          # the loss of this call; the draw counter runs on
        assert -1 <= x.max() < 1, 'generating adversarial examples should be done in [-1, 1) float domain'
        n_audios, n_channels, _ = x.size()
        assert n_channels == 1, 'Only Support Mono Audio'
        assert y.shape[0] == n_audios, 'The number of x and y should be equal'
        upper = torch.clamp(x + self.epsilon, max=1)
        lower = torch.clamp(x - self.epsilon, min=-1)
        batch_size = min(self.batch_size, n_audios)
        adver_x, success = [], []
        for batch_id, s in enumerate(range(0, n_audios, batch_size)):
            e = s + batch_size
            adver_x_batch, success_batch = self.attack_batch(x[s:e], y[s:e], lower[s:e], upper[s:e], batch_id)
            adver_x.append(adver_x_batch)
            success += success_batch
        return torch.cat(adver_x, 0), success

    def estimate_threshold_run(self, x, step=0.1):
        raise NotImplementedError('estimate_threshold is for speaker verification (a rejecting decision, a margin loss against a threshold), '
                                  'which this package has no loss for: only the SCR (speech commands) task is supported')

    def estimate_threshold(self, x, step=0.1):
        return self.estimate_threshold_run(x, step)
