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
NotImplementedError, as does generate() for task 'SV' / 'OSI' without a threshold.  Of `Kenansville` (at the end of this file, and
_KenanFFT.py) the FFT form runs; the SSA form is not provided.

`SirenAttack` (l.313-580; "SirenAttack: Generating Adversarial Audio for End-to-End Acoustic Systems", AsiaCCS 2020) is a particle swarm
on the perturbation: `n_particles` per clip, `max_epoch` epochs of `max_iter` moves, every particle scored through the EOT wrapper.
`noise_source` / `seed` / `engine` mirror FAKEBOB's:
  * 'numpy' (default) is the reference's code path: the positions, velocities, r1 and r2 are float64 arrays of numpy's global generator,
    drawn in the reference's order and shapes, the bests are updated by its host loops, and every iteration calls
    `delete_found(gbests[consider_index], ...)` with the reference's signature (tests/golden/siren.npz is recorded from the reference
    and judges this path);
  * 'device' keeps the swarm in four state tensors [clips * particles, L] on the engine and advances it with dmad_pso_init /
    dmad_pso_step / dmad_pso_update_best: the draws are Philox rows that exist in registers only, the bests are updated
    without a host loop, and the query rows go through the EOT wrapper in one call per iteration.  `_draws` counts the sample keys used
    (clips * particles per initialisation and per move) and runs on across epochs, batches and generate() calls, as NES._draws does.
    The move after the last evaluation of an epoch, whose result the reference throws away, is not made.  Statistically a reference
    run, not bit for bit one.
What both paths keep of the reference:
  * an epoch is `max_iter + 1` evaluations: the initial swarm and one after each move;
  * the convergence tests compare the mean of ALL clips' `gbests`, removed ones included, with 0.9999 times the mean remembered at the
    last test: every `abort_early_iter` iterations (ends the epoch) and every `abort_early_epoch` epochs (ends the batch);
  * particle 0 of a new epoch carries the best personal best of the last one, location and value; the others start afresh;
  * `gbest_predict` is the majority decision of the iteration in which the global best improved;
  * the result is `gbest_location + x`, and `success` is `gbests < 0`;
  * the loss is divided by the number of EOT calls once more after the EOT wrapper has averaged (as NES does).
The quirk that matters: for task 'SCR' `resolve_loss` returns unreduced cross-entropy whatever loss name is asked for (l.551 asks for
'Margin').  The swarm therefore minimises the cross-entropy of the true label, which moves AWAY from a misclassification; `gbests` is
never negative, `delete_found` never removes a clip, `success` is all False, and the driver reports 100 % robust accuracy.  That is
`loss='reference'`, the default.  `loss='margin'` is opt-in: the untargeted margin of the reference's own SEC4SR_MarginLoss
(`_utils.MarginLoss`: score_real + confidence - max other score; the sign flipped when targeted), negative for a misclassified clip, with
which the removal and `success` are live.
"""
import numpy as np
import torch

from ._EOT import EOT
from ._NES import NES
from ._utils import MarginLoss, resolve_loss, resolve_prediction

__all__ = ['FAKEBOB', 'SirenAttack', 'Kenansville']


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


SWARM_NOISE_SOURCES = ('numpy', 'device')
SIREN_LOSSES = ('reference', 'margin')


class SirenAttack:

    def __init__(self, model, threshold=None, task='CSI', targeted=False, confidence=0., epsilon=0.002, max_epoch=300, max_iter=30,
                 c1=1.4961, c2=1.4961, n_particles=25, w_init=0.9, w_end=0.1, batch_size=1, EOT_size=1, EOT_batch_size=1, verbose=1,
                 abort_early=True, abort_early_iter=10, abort_early_epoch=10, noise_source='numpy', seed=0, engine=None, loss='reference'):
        if noise_source not in SWARM_NOISE_SOURCES:
            raise ValueError('noise_source must be one of %s, not %r' % (SWARM_NOISE_SOURCES, noise_source))
        if loss not in SIREN_LOSSES:
            raise ValueError('loss must be one of %s, not %r' % (SIREN_LOSSES, loss))
        self.model = model
        self.threshold = threshold
        self.task = task
        self.targeted = targeted
        self.confidence = confidence
        self.epsilon = epsilon
        self.max_epoch = max_epoch
        self.max_iter = max_iter
        self.c1 = c1
        self.c2 = c2
        self.n_particles = n_particles
        self.w_init = w_init
        self.w_end = w_end
        self.batch_size = batch_size
        self.EOT_size = EOT_size
        self.EOT_batch_size = EOT_batch_size
        self.verbose = verbose
        self.abort_early = abort_early
        self.abort_early_iter = abort_early_iter
        self.abort_early_epoch = abort_early_epoch
        self.noise_source = noise_source
        self.seed = int(seed)
        self.loss_name = loss
        self._draws = 0                              # sample keys of the device draws used so far: see the module docstring
        self.engine = self._find_engine(engine) if noise_source == 'device' else engine

    def _find_engine(self, engine):
        from dmad_hip._lib import DmadError
        if engine is None:
            classifier = getattr(self.model, 'classifier', None)
            engine = getattr(classifier, '__dict__', {}).get('engine')
        if engine is None:
            raise DmadError("SirenAttack(noise_source='device') needs an engine: none is bound to model.classifier and no engine= was passed")
        return engine

    def _inertia(self, it):
        return (self.w_init - self.w_end) * (self.max_iter - it - 1) / self.max_iter + self.w_end

    def _evaluate(self, queries, y_batch, n):
        """Every particle through the EOT wrapper in one call -> (loss [n, P], majority decision [n, P] as a numpy array)."""
        labels = torch.as_tensor(y_batch, device=queries.device).long().repeat_interleave(self.n_particles)
        _, loss, _, decisions = self.EOT_wrapper(queries, labels)
        again = int(self.EOT_wrapper.EOT_size // self.EOT_wrapper.EOT_batch_size)
        return (loss / again).view(n, -1), resolve_prediction(decisions).reshape(n, -1)

    def _converged(self, gbests, remembered):
        return bool(torch.mean(gbests) > 0.9999 * torch.mean(remembered))

    # ---------------------------------------------------------------------------------------------------- one batch, host draws
    @staticmethod
    def _uniform(low, high, n, particles):
        """np.random.uniform between two [n, 1, L] tensors for `particles` particles per clip, as the reference draws it: float64
        [n, particles, 1, L], rounded to fp32 on the way to the device."""
        draws = np.random.uniform(low=low.unsqueeze(1).cpu().numpy(), high=high.unsqueeze(1).cpu().numpy(),
                                  size=(n, particles) + tuple(low.shape[1:]))
        return torch.tensor(draws, device=low.device, dtype=torch.float)

    def attack_batch(self, x_batch, y_batch, lower, upper, batch_id):
        if self.noise_source == 'device':
            return self._attack_batch_device(x_batch, y_batch, lower, upper, batch_id)
        with torch.no_grad():
            P = self.n_particles
            x_origin = x_batch.clone()
            n_audios, n_channels, N = x_batch.shape
            consider_index = list(range(n_audios))             # position in the working batch -> clip of x_batch
            gbest_location = torch.zeros_like(x_batch, dtype=torch.float)
            gbests = torch.full((n_audios,), np.inf, device=x_batch.device, dtype=torch.float)
            gbest_predict = np.array([None] * n_audios)
            prev_gbest, prev_gbest_epoch = gbests.clone(), gbests.clone()
            go_on = True
            for epoch in range(self.max_epoch):
                if not go_on:
                    break
                k = len(consider_index)
                if epoch == 0:
                    pbest_locations = self._uniform(lower, upper, n_audios, P)
                    pbests = torch.full((n_audios, P), np.inf, device=x_batch.device, dtype=torch.float)
                else:                                          # particle 0 carries the best personal best, the others start afresh
                    best = torch.argmin(pbests, dim=1)
                    rows = np.arange(k)
                    carried = pbest_locations[rows, best]
                    pbest_locations = torch.cat((carried.unsqueeze(1), self._uniform(lower, upper, k, P - 1)), dim=1)
                    fresh = torch.full((k, P - 1), np.inf, device=x_batch.device, dtype=torch.float)
                    pbests = torch.cat((pbests[rows, best].unsqueeze(1), fresh), dim=1)
                locations = pbest_locations.clone()
                v_upper = torch.abs(lower - upper)
                velocities = self._uniform(-v_upper, v_upper, k, P)

                epoch_go_on = True
                for it in range(self.max_iter + 1):
                    if not epoch_go_on:
                        break
                    k = len(consider_index)
                    loss, predict = self._evaluate((locations + x_batch.unsqueeze(1)).view(-1, n_channels, N), y_batch, k)
                    better = torch.where(loss < pbests)
                    for ii, jj in zip(better[0].cpu().numpy().tolist(), better[1].cpu().numpy().tolist()):
                        pbests[ii, jj] = loss[ii, jj]
                        pbest_locations[ii, jj, ...] = locations[ii, jj, ...]
                    best = torch.argmin(pbests, 1)
                    for kk in range(k):
                        index = consider_index[kk]
                        if pbests[kk, best[kk]] < gbests[index]:
                            gbests[index] = pbests[kk, best[kk]]
                            gbest_location[index] = pbest_locations[kk, best[kk]]
                            gbest_predict[index] = predict[kk, best[kk]]
                    if self.verbose:
                        print('batch: {}, epoch: {}, iter: {}, y: {}, y_pred: {}, gbest: {}'.format(
                            batch_id, epoch, it, y_batch.cpu().numpy().tolist(), gbest_predict[consider_index],
                            gbests[consider_index].cpu().numpy().tolist()))
                    if self.abort_early and (it + 1) % self.abort_early_iter == 0:
                        if self._converged(gbests, prev_gbest):
                            print('Converge, Break Inner Loop')
                            epoch_go_on = False                # the move below is still made, as in the reference
                        prev_gbest = gbests.clone()

                    # clips whose global best went negative are done (never, with cross-entropy)
                    x_batch, y_batch, lower, upper, pbest_locations, locations, velocities, pbests, consider_index = self.delete_found(
                        gbests[consider_index], x_batch, y_batch, lower, upper, pbest_locations, locations, velocities, pbests, consider_index)
                    if len(consider_index) == 0:
                        go_on = False
                        break
                    if it < self.max_iter:
                        shape = (len(consider_index), P, n_channels, N)
                        r1 = torch.tensor(np.random.rand(*shape) + 0.00001, device=x_batch.device, dtype=torch.float)
                        r2 = torch.tensor(np.random.rand(*shape) + 0.00001, device=x_batch.device, dtype=torch.float)
                        velocities = (self._inertia(it) * velocities + self.c1 * r1 * (pbest_locations - locations) +
                                      self.c2 * r2 * (gbest_location[consider_index, ...].unsqueeze(1) - locations))
                        locations = locations + velocities
                        locations = torch.min(torch.max(locations, lower.unsqueeze(1)), upper.unsqueeze(1))

                if self.abort_early and (epoch + 1) % self.abort_early_epoch == 0:
                    if self._converged(gbests, prev_gbest_epoch):
                        print('Converge, Break Outer Loop')
                        go_on = False
                    prev_gbest_epoch = gbests.clone()
            return gbest_location + x_origin, [bool(g < 0) for g in gbests]

    def delete_found(self, gbests, x_batch, y_batch, lower, upper, pbest_locations, locations, volicities, pbests, consider_index):
        """Keeps the positions whose `gbests` entry is not negative (the reference's signature and order of results): the tensors
        sliced, the index list filtered; (None, ..., []) when none is left."""
        keep = [ii for ii, g in enumerate(gbests) if not g < 0]
        if not keep:
            return None, None, None, None, None, None, None, None, []
        rows = torch.as_tensor(keep, device=x_batch.device)
        pick = lambda t: t.index_select(0, rows)
        return (pick(x_batch), pick(y_batch), pick(lower), pick(upper), pick(pbest_locations), pick(locations), pick(volicities),
                pick(pbests), [consider_index[ii] for ii in keep])

    # ---------------------------------------------------------------------------------------------------- one batch, device draws
    def _attack_batch_device(self, x_batch, y_batch, lower, upper, batch_id):
        eng, P = self.engine, self.n_particles
        with torch.no_grad():
            n_audios, n_channels, N = x_batch.shape
            dev = x_batch.device
            x_origin = x_batch
            x_batch, lower, upper = x_batch.float().contiguous(), lower.float().contiguous(), upper.float().contiguous()
            y_batch = torch.as_tensor(y_batch, device=dev).long()
            consider_index = list(range(n_audios))
            index = None                                       # device twin of consider_index once a clip has been removed
            gbest_location = torch.zeros((n_audios, n_channels, N), device=dev, dtype=torch.float)
            gbests = torch.full((n_audios,), np.inf, device=dev, dtype=torch.float)
            gbest_predict = torch.full((n_audios,), -1, device=dev, dtype=torch.long)
            prev_gbest, prev_gbest_epoch = gbests.clone(), gbests.clone()
            pbests = pbest_loc = loc = vel = queries = None
            go_on = True
            for epoch in range(self.max_epoch):
                if not go_on:
                    break
                k = len(consider_index)
                if epoch == 0:
                    keep = None
                    pbests = torch.full((k, P), np.inf, device=dev, dtype=torch.float)
                else:                                          # particle 0 carries the best personal best, the others start afresh
                    best = torch.argmin(pbests, dim=1)
                    keep = pbest_loc.index_select(0, torch.arange(k, device=dev) * P + best)          # a copy: pbest_loc is rewritten
                    fresh = torch.full((k, P - 1), np.inf, device=dev, dtype=torch.float)
                    pbests = torch.cat((pbests.gather(1, best.unsqueeze(1)), fresh), dim=1).contiguous()
                pbest_loc, loc, vel, queries = eng.pso_init(x_batch, lower, upper, P, self.seed, self._draws, keep, pbest_loc, loc, vel, queries)
                self._draws += k * P

                for it in range(self.max_iter + 1):
                    loss, predict = self._evaluate(queries.view(-1, n_channels, N), y_batch, k)
                    predict = torch.as_tensor(predict.astype(np.int64), device=dev)
                    eng.pso_update_best(loss, predict, loc, pbests, pbest_loc, gbests, gbest_location, gbest_predict, index)
                    working = gbests if index is None else gbests.index_select(0, index)
                    if self.verbose:
                        print('batch: {}, epoch: {}, iter: {}, y: {}, y_pred: {}, gbest: {}'.format(
                            batch_id, epoch, it, y_batch.cpu().numpy().tolist(), gbest_predict.cpu().numpy()[consider_index], working.cpu().numpy().tolist()))
                    epoch_go_on = True
                    if self.abort_early and (it + 1) % self.abort_early_iter == 0:
                        if self._converged(gbests, prev_gbest):
                            print('Converge, Break Inner Loop')
                            epoch_go_on = False
                        prev_gbest = gbests.clone()

                    # clips whose global best went negative are done (never, with cross-entropy)
                    found = working < 0
                    if bool(found.any()):
                        rows = torch.nonzero(~found).flatten()
                        consider_index = [consider_index[ii] for ii in rows.tolist()]
                        k = len(consider_index)
                        if k == 0:
                            go_on = False
                            break
                        index = torch.as_tensor(consider_index, device=dev, dtype=torch.long)
                        x_batch, y_batch, lower, upper = (t.index_select(0, rows) for t in (x_batch, y_batch, lower, upper))
                        pbests = pbests.index_select(0, rows)
                        pbest_loc, loc, vel, queries = (t.view(-1, P, N).index_select(0, rows).view(k * P, N) for t in (pbest_loc, loc, vel, queries))
                    if not epoch_go_on or it == self.max_iter:
                        break                                  # no move after the last evaluation of an epoch: nothing would read it
                    gbest_working = gbest_location if index is None else gbest_location.index_select(0, index)
                    eng.pso_step(x_batch, lower, upper, pbest_loc, gbest_working, P, self._inertia(it), self.c1, self.c2, self.seed,
                                 self._draws, loc, vel, queries)
                    self._draws += k * P

                if self.abort_early and (epoch + 1) % self.abort_early_epoch == 0:
                    if self._converged(gbests, prev_gbest_epoch):
                        print('Converge, Break Outer Loop')
                        go_on = False
                    prev_gbest_epoch = gbests.clone()
            return gbest_location + x_origin, (gbests < 0).cpu().numpy().tolist()

    # ---------------------------------------------------------------------------------------------------------------- all clips
    def generate(self, x, y, targeted=False):
        if self.task in ('SV', 'OSI') and self.threshold is None:
            raise NotImplementedError('SirenAttack for task %s needs a decision threshold, and estimating one is speaker verification, '
                                      'which this package has no loss for' % (self.task,))
        self.targeted = targeted
        self.loss, self.grad_sign = resolve_loss('Margin', self.targeted, self.confidence, self.task, self.threshold, False)
        if self.loss_name == 'margin':
            self.loss = MarginLoss(self.targeted, self.confidence)
        self.EOT_wrapper = EOT(self.model, self.loss, self.EOT_size, self.EOT_batch_size, False)
        assert -1 <= x.max() < 1, 'generating adversarial examples should be done in [-1, 1) float domain'
        n_audios, n_channels, _ = x.size()
        assert n_channels == 1, 'Only Support Mono Audio'
        assert y.shape[0] == n_audios, 'The number of x and y should be equal'
        lower = torch.clamp(-1 - x, min=-self.epsilon)          # bounds of the perturbation, not of the adversarial clip
        upper = torch.clamp(1 - x, max=self.epsilon)
        batch_size = min(self.batch_size, n_audios)
        adver_x, success = [], []
        for batch_id, s in enumerate(range(0, n_audios, batch_size)):
            e = s + batch_size
            adver_x_batch, success_batch = self.attack_batch(x[s:e], y[s:e], lower[s:e], upper[s:e], batch_id)
            adver_x.append(adver_x_batch)
            success += success_batch
        return torch.cat(adver_x, 0), success


FFT_BACKENDS = ('torch', 'device')


class Kenansville:
    """The reference's Kenansville (l.584-663) in its default form, atk_name='fft': see _KenanFFT.py.  `fft_backend` / `engine` are this
    package's additions: 'torch' (default) runs the reference's torch.fft operators, 'device' the engine's whole-clip FFT pair and its
    bisection kernel; the engine is found as SirenAttack finds it.  atk_name='ssa', the reference's float64 SVD of a Hankel matrix on the
    CPU at batch 1, is not provided."""

    def __init__(self, model, atk_name='fft', max_iter=15, raster_width=100, early_stop=False, targeted=False, verbose=1, BITS=16, batch_size=1,
                 fft_backend='torch', engine=None):
        if atk_name == 'ssa':
            raise NotImplementedError("Kenansville(atk_name='ssa') is the reference's CPU SVD form (a float64 SVD of a Hankel matrix per clip, "
                                      "at batch 1), which this package does not provide: the FFT form, atk_name='fft', runs")
        if atk_name != 'fft':
            raise ValueError("atk_name must be 'fft' (or 'ssa', which is not provided), not %r" % (atk_name,))
        if fft_backend not in FFT_BACKENDS:
            raise ValueError('fft_backend must be one of %s, not %r' % (FFT_BACKENDS, fft_backend))
        self.model = model
        self.atk_name = atk_name
        self.max_iter = max_iter
        self.raster_width = raster_width           # of the SSA form; unused by the FFT form, as in the reference
        self.targeted = targeted
        self.verbose = verbose
        self.BITS = BITS
        self.early_stop = early_stop
        self.batch_size = batch_size
        self.fft_backend = fft_backend
        self.engine = self._find_engine(engine) if fft_backend == 'device' else engine
        self.trace = None                          # a list here receives (factors, predictions) per iteration (_KenanFFT.atk_bst_fft)

    def _find_engine(self, engine):
        from dmad_hip._lib import DmadError
        if engine is None:
            classifier = getattr(self.model, 'classifier', None)
            engine = getattr(classifier, '__dict__', {}).get('engine')
        if engine is None:
            raise DmadError("Kenansville(fft_backend='device') needs an engine: none is bound to model.classifier and no engine= was passed")
        return engine

    @torch.no_grad()
    def _scores(self, x):
        """The system's scores [n, C] of one evaluation per clip: the one-call query where the system has one (as _EOT.EOT asks), else
        the forward pass."""
        if hasattr(self.model, 'query'):
            return self.model.query(x, 1, per_call=1)[0][0]
        return self.model(x)

    def attack_batch(self, x_batch, y_batch, batch_id, fs=16_000):
        from ._KenanFFT import atk_bst_fft
        return atk_bst_fft(x_batch, y_batch, self.targeted, self._scores, self.max_iter, self.verbose, backend=self.fft_backend,
                           engine=self.engine, trace=self.trace)

    def generate(self, x, y, targeted=False, fs=16_000):
        self.targeted = targeted
        n_audios, n_channels, _ = x.size()
        assert n_channels == 1, 'Only Support Mono Audio'
        assert y.shape[0] == n_audios, 'The number of x and y should be equal'
        batch_size = min(self.batch_size, n_audios)
        adver_x, success = [], []
        for batch_id, s in enumerate(range(0, n_audios, batch_size)):
            e = s + batch_size
            adver_x_batch, success_batch = self.attack_batch(x[s:e], y[s:e], batch_id, fs=fs)
            adver_x.append(adver_x_batch)
            success += success_batch
        return torch.cat(adver_x, 0), success
