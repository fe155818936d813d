"""NES gradient estimate for the query-only attack drivers (behaviour of the reference's robustness_eval/_NES.py:15-55;
caller black_box_attack.py:186-190).

For every clip: `samples_per_draw` antithetic Gaussian probes x +- sigma * u (the first draw batch also carries the
unperturbed clip in slot 0), each scored through the EOT wrapper; the estimate is  grad = E[loss * u] / sigma.
Returns (mean probe loss [n], grad [n,1,L], loss of the unperturbed clip [n], its scores [n,C], its majority decision [n]).
One quirk of the reference is part of the contract and kept: the EOT wrapper already returns means over its model
calls, and NES divides them by the number of EOT calls once more (ref l.33-35).

`noise_source`:
  * 'torch' (default): the reference's code path — the directions come from torch's generator as one [n, P/2, 1, L] tensor, the queries
    are one [n * (P + 1), 1, L] batch.
  * 'device': the directions are Philox rows keyed (seed, _draws + b * P/2 + j, stream NES) that never exist in memory.
    The queries are made `probe_rows` rows at a time by Engine.nes_probes (default: the engine's max_batch), each chunk goes through
    the EOT wrapper, and the estimate is one Engine.nes_grad call per draw batch, which regenerates the directions in registers.
    The engine is the one of `EOT_wrapper.model.classifier` (where AcousticSystem._engine_chain finds it), or `engine=`.  `_draws`
    advances by n * P/2 per draw batch, as the purifiers' counters do.  Statistically a reference run, not bit for bit one."""
import torch
import torch.nn as nn

from ._utils import resolve_prediction

NOISE_SOURCES = ('torch', 'device')


class NES(nn.Module):

    def __init__(self, samples_per_draw, samples_per_draw_batch, sigma, EOT_wrapper, noise_source='torch', seed=0, probe_rows=None,
                 engine=None):
        super().__init__()
        if noise_source not in NOISE_SOURCES:
            raise ValueError('noise_source must be one of %s, not %r' % (NOISE_SOURCES, noise_source))
        self.samples_per_draw = samples_per_draw
        self.samples_per_draw_batch_size = samples_per_draw_batch
        self.sigma = sigma
        self.EOT_wrapper = EOT_wrapper
        self.noise_source = noise_source
        self.seed = int(seed)
        self.probe_rows = probe_rows
        self._draws = 0
        self.engine = self._find_engine(engine) if noise_source == 'device' else engine

    def _find_engine(self, engine):
        from dmad_hip._lib import DmadError
        if engine is None:
            classifier = getattr(getattr(self.EOT_wrapper, 'model', None), 'classifier', None)
            engine = getattr(classifier, '__dict__', {}).get('engine')
        if engine is None:
            raise DmadError("NES(noise_source='device') needs an engine: none is bound to EOT_wrapper.model.classifier and no engine= was passed")
        return engine

    def _probe(self, x, y, with_origin):
        """One draw batch -> (u [n, P, 1, L] probe directions, loss [n, P(+1)], scores [n, P(+1), C], decisions)."""
        n, ch, L = x.shape
        half = torch.randn([n, self.samples_per_draw_batch_size // 2, ch, L], device=x.device)
        u = torch.cat((half, -half), 1)
        probes = torch.cat((torch.zeros_like(x).unsqueeze(1), u), 1) if with_origin else u
        per_clip = probes.shape[1]
        queries = (probes * self.sigma + x.unsqueeze(1)).view(-1, ch, L)
        labels = torch.as_tensor(y, device=x.device).long().repeat_interleave(per_clip)
        scores, loss, _, decisions = self.EOT_wrapper(queries, labels)
        again = int(self.EOT_wrapper.EOT_size // self.EOT_wrapper.EOT_batch_size)
        return u, (loss / again).view(n, per_clip), (scores / again).view(n, per_clip, -1), decisions

    def _probe_device(self, x, y, with_origin, draw0):
        """One draw batch on the engine's probe keys -> (loss [n, P(+1)], scores [n, P(+1), C], decisions); at most `probe_rows` query
        rows exist at a time."""
        eng = self.engine
        n, ch, L = x.shape
        assert ch == 1, 'Only Support Mono Audio'
        P = self.samples_per_draw_batch_size
        per_clip = P + int(with_origin)
        total = n * per_clip
        step = int(self.probe_rows or eng.max_batch)
        labels = torch.as_tensor(y, device=x.device).long().repeat_interleave(per_clip)
        scores, loss, decisions = [], [], []
        for r0 in range(0, total, step):
            rows = min(step, total - r0)
            queries = eng.nes_probes(x, P, self.sigma, with_origin, self.seed, draw0, r0, rows).view(rows, 1, L)
            s, l, _, d = self.EOT_wrapper(queries, labels[r0:r0 + rows])
            scores.append(s)
            loss.append(l)
            decisions += d
        again = int(self.EOT_wrapper.EOT_size // self.EOT_wrapper.EOT_batch_size)
        return (torch.cat(loss) / again).view(n, per_clip), (torch.cat(scores) / again).view(n, per_clip, -1), decisions

    def _forward_device(self, x, y):
        n, _, L = x.shape
        P = self.samples_per_draw_batch_size
        draws = self.samples_per_draw // P
        scale = 1.0 / (P * self.sigma * draws)                   # the mean over the P probes, / sigma / draws (ref l.47,54)
        grad = mean_loss = None
        for i in range(draws):
            draw0 = self._draws
            loss, scores, decisions = self._probe_device(x, y, i == 0, draw0)
            self._draws += n * (P // 2)
            if i == 0:
                adver_loss, adver_score = loss[:, 0], scores[:, 0, :]
                predict = resolve_prediction(decisions).reshape(n, -1)[:, 0]
                loss = loss[:, 1:]
            grad = self.engine.nes_grad(loss, P, scale, self.seed, draw0, grad)
            mean_loss = loss.mean(1) if mean_loss is None else mean_loss + loss.mean(1)
        return mean_loss / draws, grad.view(n, 1, L), adver_loss, adver_score, predict

    def forward(self, x, y):
        if self.noise_source == 'device':
            return self._forward_device(x, y)
        n = x.shape[0]
        draws = self.samples_per_draw // self.samples_per_draw_batch_size
        u, loss, scores, decisions = self._probe(x, y, with_origin=True)
        adver_loss, adver_score = loss[:, 0], scores[:, 0, :]
        predict = resolve_prediction(decisions).reshape(n, -1)[:, 0]
        loss = loss[:, 1:]
        grad = (loss[:, :, None, None] * u).mean(1)
        mean_loss = loss.mean(1)
        for _ in range(1, draws):
            u, loss, _, _ = self._probe(x, y, with_origin=False)
            grad += (loss[:, :, None, None] * u).mean(1)
            mean_loss += loss.mean(1)
        return mean_loss / draws, grad / self.sigma / draws, adver_loss, adver_score, predict
