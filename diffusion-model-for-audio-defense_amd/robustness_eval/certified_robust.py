"""Host mirror of robustness_eval/certified_robust.py (RobustCertificate, ref l.6-127) on the MI355X
engine.  Same constructor, methods, return types and assertions as the reference.

What changes underneath:
  * smooth_predict's Monte Carlo loop (ref l.33-67) runs as ONE call into libdmad_hip.so
    (dmad_smooth_votes) when denoiser / transform / classifier are this package's HIP-backed stages:
    noise, sqrt(alpha_bar*) scaling, one-shot DiffWave purification, mel-dB, VGG19_bn, arg-max and the
    per-class histogram never leave the GPU and the 10 `.item()` syncs of the reference become one
    80-byte copy.  Without a denoiser (the plain randomized-smoothing baseline) the loop is one call too:
    dmad_rs_smooth_votes behind the HIP mel front-end and a HIP-backed classifier, dmad_m5_rs_smooth_votes for
    an M5 on the engine.  Other classifiers / transforms (a default M5, user modules) are called as torch
    modules on the purified batch and only the vote count runs in HIP.
  * The N samples shard over torch.distributed ranks (one process per GPU); the per-class counts are
    summed with a single all_reduce (RCCL over xGMI on MI355X).  With device noise (Philox keyed by the
    global sample index) the counts do not depend on the number of ranks.
  * noise_source='torch_cpu' reproduces the reference's CPU torch.normal stream exactly (parity).
  * lower_conf_bound uses scipy's Beta quantile; the reference's statsmodels call
    proportion_confint(k, n, alpha=2*alpha, method='beta')[0] is the same Clopper-Pearson bound.
"""
import math

import torch
from scipy.stats import beta as _beta
from scipy.stats import norm

__all__ = ['RobustCertificate']


def _dist():
    import torch.distributed as dist
    if dist.is_available() and dist.is_initialized():
        return dist, dist.get_rank(), dist.get_world_size()
    return None, 0, 1


class RobustCertificate():

    def __init__(self, classifier: torch.nn.Module, transform=None, denoiser=None, one_shot_rev: bool = False,
                 num_classes=10, noise_source: str = 'device', seed: int = None, shard: bool = True, calibrate: int = 0,
                 calibrate_clips: int = 3, log=None) -> None:
        self.classifier = classifier
        self.transform = transform
        self.denoiser = denoiser
        self.num_classes = num_classes
        self.one_shot_rev = one_shot_rev
        assert noise_source in ('device', 'torch_cpu')
        self.noise_source = noise_source
        self.seed = seed
        self.shard = shard
        self._calls = 0
        # calibrate = n > 0: before the fused smooth_predict of the first `calibrate_clips` clips at each sigma, measure the
        # recheck bounds of the exact-vote engine for the resident weights on n samples of the clip at hand
        # (Engine.calibrate_recheck: it can only WIDEN a bound, never go below the committed defaults) — the defaults were
        # measured on the synthetic VGG19_bn; the certification driver switches it on (real checkpoints).  `log`: callable
        # that receives one line per calibration / audit (the driver passes its logger).
        self.calibrate = int(calibrate)
        self.calibrate_clips = max(1, int(calibrate_clips))
        self._calibrated = {}                   # t -> (tau1, tau2, e1, e2): the widest bounds / largest errors seen so far
        self._calibrated_clips = {}             # t -> fingerprints of the clips measured (certify() calls smooth_predict twice per clip)
        self.log = log
        self._last = None                       # (seed, sigma, coeffs, n) of the last fused smooth_predict, for audit()
        self.audit_log = []                     # one dict per audited smooth_predict

    # ------------------------------------------------------------------------------------------
    def _fused(self):
        """True when every stage is HIP-backed and lives in one engine."""
        from dmad_hip.transforms import MelSpectrogramDB
        den, cls, tr = self.denoiser, self.classifier, self.transform
        eng = getattr(den, 'engine', None)
        is_mel_db = isinstance(tr, MelSpectrogramDB)
        if not is_mel_db:       # the reference's own Compose([MelSpectrogram, AmplitudeToDB]) through the opt-in shims
            stages = [getattr(t, '_dmad_stage', None) for t in getattr(tr, 'transforms', [])]
            is_mel_db = stages == ['mel_power', 'power_to_db']
        if eng is not None and is_mel_db and 'engine' not in getattr(cls, '__dict__', {}) and hasattr(cls, 'bind_engine'):
            from dmad_hip._lib import DmadError
            try:
                cls.bind_engine(eng)                        # HIP-backed classifier not yet bound: bind it to the denoiser's engine
            except DmadError:                               # that engine serves another classifier: stay unfused
                cls.bind_engine()
        return (eng is not None and is_mel_db and getattr(cls, 'engine', None) is eng and eng.has_classifier and eng.has_wavenet)

    def _fused_spec(self):
        """The engine that runs the spec-domain loop (BASELINE C5) in one call: no waveform denoiser, transform = SpecDefense(mel,
        Improved-Diffusion purifier), every stage HIP-backed on ONE engine, device noise.  None otherwise."""
        if self.denoiser is not None or self.noise_source != 'device':
            return None
        from diffusion_models.improved_diffusion_ddpm import SpecDefense
        from dmad_hip.transforms import MelSpectrogramDB
        tr, cls = self.transform, self.classifier
        if not isinstance(tr, SpecDefense) or not isinstance(tr.mel, MelSpectrogramDB):
            return None
        eng = tr.mel.engine
        model = tr.purifier.model
        if getattr(model, '__dict__', {}).get('engine') is not eng:      # the HIP UNet keeps its engine in __dict__ once bound
            return None
        if hasattr(cls, 'bind_engine') and 'engine' not in getattr(cls, '__dict__', {}):
            from dmad_hip._lib import DmadError
            try:
                cls.bind_engine(eng)
            except DmadError:
                return None
        return eng if (getattr(cls, 'engine', None) is eng and eng.has_classifier and eng.has_unet) else None

    def _fused_rs(self):
        """The plain randomized-smoothing loop (denoiser=None, the driver's --defense_method randsmooth) as one engine call:
        ('mel', engine) when the transform is the HIP mel front-end and the classifier is HIP-backed and bound to its engine (an unbound
        one is bound to it first; if that engine serves another classifier it gets one of its own and the loop stays unfused, as in
        _fused()), ('m5', engine) when there is no transform and the classifier is an M5 that use_engine() put on an engine.  None
        otherwise: a user's torch module, a default M5 or any other transform keep the host loop."""
        if self.denoiser is not None:
            return None
        cls, tr = self.classifier, self.transform
        if getattr(cls, 'training', False):                 # the host loop runs (or refuses) a module in training mode as it is
            return None
        if tr is None:
            from audio_models.M5.M5Net import is_m5
            eng = getattr(cls, '__dict__', {}).get('engine')
            return ('m5', eng) if is_m5(cls) and eng is not None and eng.has_m5 else None
        if not hasattr(cls, 'bind_engine'):
            return None
        from dmad_hip.transforms import MelSpectrogramDB
        if isinstance(tr, MelSpectrogramDB):
            eng = tr.engine
        else:                   # the reference's own Compose([MelSpectrogram, AmplitudeToDB]) through the opt-in shims
            stages = getattr(tr, 'transforms', [])
            if [getattr(t, '_dmad_stage', None) for t in stages] != ['mel_power', 'power_to_db']:
                return None
            eng = stages[0].engine
        if 'engine' not in getattr(cls, '__dict__', {}):
            from dmad_hip._lib import DmadError
            try:
                cls.bind_engine(eng)
            except DmadError:                               # that engine serves another classifier: stay unfused
                cls.bind_engine()
        return ('mel', eng) if getattr(cls, 'engine', None) is eng and eng.has_classifier else None

    @staticmethod
    def _rs_votes(route, x, sigma, n, seed, sample0, delta, counts):
        """n samples from global index sample0 on the route _fused_rs() gave, added to counts (None: fresh counts).  The passes are the
        engine's max_batch, not the caller's batch_size: a sample's logits do not depend on the batch it ran in."""
        kind, eng = route
        if kind == 'm5':
            return eng.m5_rs_smooth_votes(x, sigma, n, seed=seed, sample0=sample0, delta=delta, counts=counts)[0]
        return eng.rs_smooth_votes(x, sigma, n, seed=seed, sample0=sample0, delta=delta, counts=counts)[0]

    @torch.no_grad()
    def forward(self, x: torch.Tensor):
        x_in = x
        if self.denoiser is not None:
            x_in = self.denoiser.one_shot_denoise(x_in)
        if self.transform is not None:
            x_in = self.transform(x_in)
        return self.classifier(x_in)

    def _seed_for_call(self):
        if self.noise_source != 'device':
            return 0                            # the CPU generator must not be touched before the torch.normal draws
        if self.seed is not None:
            s = (int(self.seed) * 1000003 + self._calls) & 0xFFFFFFFFFFFFFFFF
        else:                                   # governed by torch.manual_seed, identical on every rank only
            s = int(torch.randint(0, 2 ** 62, (1,)).item())   # if the ranks seeded torch identically
            dist, _, world = _dist()
            if dist is not None and world > 1:
                t = torch.tensor([s], dtype=torch.int64, device='cuda' if torch.cuda.is_available() and dist.get_backend() == 'nccl' else 'cpu')
                dist.broadcast(t, 0)
                s = int(t.item())
        self._calls += 1
        return s

    @torch.no_grad()
    def smooth_predict(self, x: torch.Tensor, num_sampling: int = 100, sigma=0.25, batch_size=64):
        assert(x.shape[0] == 1)
        dist, rank, world = _dist()
        if not self.shard:
            dist, rank, world = None, 0, 1
        # contiguous shard of the global sample index range for this rank
        lo = (num_sampling * rank) // world
        hi = (num_sampling * (rank + 1)) // world
        seed = self._seed_for_call()

        coeffs = None
        if self.denoiser is not None:
            if hasattr(getattr(self.denoiser, 'model', None), 'any_length'):      # a DiffWave mirror: the vote loops run at clip_len only
                from diffusion_models.diffwave_ddpm import fixed_length_only
                fixed_length_only(self.denoiser.model, x, 'the vote loop (RobustCertificate.smooth_predict)')
            alpha_bar_star = 1 / (1 + sigma ** 2)
            t_star = self.compute_t_star(alpha_bar_star)
            self.denoiser.reverse_timestep = t_star
            Alpha_bar = self.denoiser.diffusion_hyperparams['Alpha_bar']
            t = t_star - 1
            coeffs = (t, float((1 / Alpha_bar).sqrt()[t]), float((1 / Alpha_bar - 1).sqrt()[t]),
                      float(torch.tensor(alpha_bar_star ** 0.5, dtype=torch.float32)))

        fused = self._fused()
        if fused and self.calibrate > 0 and getattr(self.denoiser.engine, 'precision', None) == 2:      # EXACT engines
            eng, tk = self.denoiser.engine, coeffs[0]
            self._calibrate_clip(
                x, tk, lambda: eng.calibrate_recheck(x, sigma, coeffs[3], tk, coeffs[1], coeffs[2], n=self.calibrate,
                                                     n_fp32=max(16, self.calibrate // 2)),
                eng.set_recheck_margin, eng.set_recheck_margin2,
                lambda c, r: 'recheck bounds at sigma=%g (t*=%d), clip %d of %d: observed 16-bit error %.4g, split-f16 error %.3g -> tau1 %.4g, '
                             'tau2 %.3g' % (sigma, tk + 1, c, self.calibrate_clips, r[2], r[3], r[0], r[1]))
        self._last = (seed, sigma, coeffs, num_sampling) if (fused and self.noise_source == 'device') else None
        spec_eng = self._fused_spec() if not fused else None
        spec_args = None
        if spec_eng is not None:
            from diffusion_models.Improved_Diffusion_Unconditional.improved_diffusion.sc09_spectrogram_dataset import MEL_LOWER_BOUND, MEL_UPPER_BOUND
            spec_args = tuple(self.transform.purifier.purify_coefficients()) + (MEL_LOWER_BOUND, MEL_UPPER_BOUND)
            exact = getattr(spec_eng, 'precision', None) == 2 and spec_eng.mode == 1           # DMAD_EXACT engine in DMAD_MODE_EXACT_VOTES
            if exact and self.calibrate > 0:        # the spec tiers' bounds for the resident weights at this (sigma, t*)
                def measure():
                    tau, e_, s_ = spec_eng.calibrate_spec_recheck(x, sigma, spec_args, n=max(64, min(self.calibrate, 512)))
                    return tau, spec_eng.spec_recheck_margin2, e_, s_
                self._calibrate_clip(
                    x, ('spec', spec_args[0], round(float(sigma), 6)), measure, spec_eng.set_spec_recheck_margin, spec_eng.set_spec_recheck_margin2,
                    lambda c, r: 'spec-tier recheck bound at sigma=%g (t*=%d), clip %d of %d: observed 16-bit chain error %.4g (scale %.3g) -> '
                                 'tau_spec %.4g, tau_spec2 %.3g' % (sigma, spec_args[0], c, self.calibrate_clips, r[2], r[3], r[0], r[1]))
            if exact and self.noise_source == 'device':
                self._last = ('spec', seed, sigma, spec_args, num_sampling)
        rs = self._fused_rs() if (not fused and spec_eng is None and x.is_cuda) else None
        if self.noise_source == 'torch_cpu':
            # The reference's stream: one CPU torch.normal draw per batch (ref l.47).  The stream is batch-split invariant,
            # so every rank draws the whole stream, keeps its own slice of each batch and feeds it to the engine batch by
            # batch: host and device hold one batch of noise at a time (64 kB per sample), whatever num_sampling is.
            counts, done = None, 0
            while done < num_sampling:
                b = min(batch_size, num_sampling - done)
                d = torch.normal(0, sigma, size=(b,) + tuple(x.shape))
                a, e = max(lo, done), min(hi, done + b)
                if e > a:
                    delta = d[a - done:e - done].to(x.device)
                    if fused:
                        counts, _, _ = self.denoiser.engine.smooth_votes(x, sigma, coeffs[3], coeffs[0], coeffs[1], coeffs[2], e - a,
                                                                         seed=seed, sample0=a, delta=delta, counts=counts)
                    elif rs is not None:
                        counts = self._rs_votes(rs, x, sigma, e - a, seed, a, delta, counts)
                    else:
                        c = self._generic_votes(x, sigma, coeffs, a, e, seed, delta, batch_size)
                        counts = c if counts is None else counts + c
                done += b
            if counts is None:
                counts = torch.zeros(self.num_classes, dtype=torch.int64, device=x.device)
        elif spec_eng is not None and hi > lo:
            counts, _, _ = spec_eng.spec_smooth_votes(x, sigma, *spec_args, hi - lo, batch=batch_size, seed=seed, sample0=lo)
        elif fused and hi > lo:
            counts, _, _ = self.denoiser.engine.smooth_votes(x, sigma, coeffs[3], coeffs[0], coeffs[1], coeffs[2], hi - lo,
                                                             seed=seed, sample0=lo)
        elif rs is not None and hi > lo:
            counts = self._rs_votes(rs, x, sigma, hi - lo, seed, lo, None, None)
        else:
            counts = self._generic_votes(x, sigma, coeffs, lo, hi, seed, None, batch_size)

        if dist is not None and world > 1:
            if dist.get_backend() != 'nccl':
                counts = counts.cpu()
            dist.all_reduce(counts)                 # the single collective of the path: int64[num_classes]
        return counts.cpu()

    def _calibrate_clip(self, x, key, measure, set_tau1, set_tau2, line):
        """The per-clip recheck calibration of either vote loop at `key` (t for the waveform loop, ('spec', t*, sigma) for the spec
        loop).  The first `calibrate_clips` distinct clips of a key are measured — certify() calls smooth_predict twice per clip —
        by measure() -> (tau1, tau2, errors...), the engine's calibration (it can only WIDEN a bound); the key keeps the elementwise
        maximum of what its clips gave, and both of its bounds are installed on every visit (another key may have run in between).
        line(clip number, record) is the log line of a measurement."""
        seen = self._calibrated_clips.setdefault(key, [])
        fp = self._clip_fingerprint(x)
        if fp not in seen and len(seen) < self.calibrate_clips:
            new, old = measure(), self._calibrated.get(key)
            self._calibrated[key] = new if old is None else tuple(max(a, b) for a, b in zip(new, old))
            seen.append(fp)
            if self.log is not None:
                self.log(line(len(seen), self._calibrated[key]))
        if key in self._calibrated:
            set_tau1(self._calibrated[key][0], calibrated=True)
            set_tau2(self._calibrated[key][1], calibrated=True)

    def _generic_votes(self, x, sigma, coeffs, lo, hi, seed, delta, batch_size):
        """Purify with the HIP one-shot, then call the caller's transform / classifier modules."""
        device = x.device
        counts = None
        cls = self.classifier
        if hasattr(cls, 'bind_engine') and 'engine' not in getattr(cls, '__dict__', {}) and x.is_cuda:
            cls.bind_engine()                   # HIP-backed classifiers bind lazily in forward(): the vote / noise kernels need it now
        eng = getattr(self.denoiser, 'engine', None) or getattr(cls, 'engine', None)
        pos = lo
        while pos < hi:
            b = min(batch_size, hi - pos)
            x_in = x.repeat(b, 1, 1)
            if delta is not None:
                d = delta[pos - lo:pos - lo + b]
            else:
                if eng is None:
                    raise RuntimeError('device noise needs a HIP-backed denoiser or classifier; use noise_source="torch_cpu"')
                d = sigma * eng.philox_normal(seed, pos, 0, b).reshape(b, *x.shape)
            x_in = x_in + d
            if self.denoiser is not None:
                x_in = coeffs[3] * x_in
            out = self.forward(x_in)
            if counts is None:
                counts = torch.zeros(out.shape[-1], dtype=torch.int64, device=device)
            if eng is not None and out.is_cuda and out.shape[-1] == eng.num_classes:
                eng.vote(out, counts)
            else:
                pred = out.max(1, keepdim=True)[1].reshape(-1)
                counts += torch.bincount(pred, minlength=out.shape[-1]).to(counts.dtype)
            pos += b
        if counts is None:
            counts = torch.zeros(self.num_classes, dtype=torch.int64, device=device)
        return counts

    @staticmethod
    def _clip_fingerprint(x: torch.Tensor) -> str:
        import hashlib
        return hashlib.sha1(x.detach().float().cpu().contiguous().numpy().tobytes()).hexdigest()

    @torch.no_grad()
    def audit(self, x: torch.Tensor, k: int):
        """Opt-in check of the exact-vote mode on the LAST fused smooth_predict(x, ...) of either loop: k of its Monte Carlo samples
        (drawn without replacement from the global index range, the same on every rank) are evaluated on the loop's first pass (the
        16-bit tier, in the exact-vote mode whatever the engine's mode); those that VOTED there (margin >= the recheck bound) are
        re-evaluated on the split-f16 tier (fp32-grade) from the same Philox keys, and every sample whose arg-max differs is
        reported.  Returns (and appends to self.audit_log) a dict: audited, voted_on_tier1, disagreements [(sample index, tier-1
        class, tier-2 class, tier-1 margin)], largest leader-difference error seen, the bound (tau1; spec loop: tau_spec, loop)."""
        if self._last is None:
            raise RuntimeError('audit() follows a fused smooth_predict with device noise on an exact-vote engine')
        spec = self._last[0] == 'spec'
        if spec:
            _, seed, sigma, spec_args, n = self._last
            eng = self._fused_spec()
            tau, tau_key, unet = eng.spec_recheck_margin, 'tau_spec', ' UNet'

            def evaluate(idx, tier):            # the UNet's 16-bit (1) / split-f16 (2) tier
                return eng.spec_eval_samples(x, sigma, *spec_args, idx, tier=tier, seed=seed)
        else:
            seed, sigma, coeffs, n = self._last
            eng = self.denoiser.engine
            tau, tau_key, unet = eng.recheck_margin, 'tau1', ''

            def evaluate(idx, tier):            # path 0 = the loop's first pass (16-bit WaveNet + the classifier tier it runs), 2 = split-f16
                return eng.eval_samples(x, sigma, coeffs[3], coeffs[0], coeffs[1], coeffs[2], idx, path=0 if tier == 1 else 2, seed=seed)
        if getattr(eng, 'precision', None) != 2:
            raise RuntimeError('audit() needs an exact-vote (DMAD_EXACT) engine')
        k = min(int(k), n)
        g = torch.Generator().manual_seed(seed & 0x7FFFFFFFFFFFFFFF)
        idx = torch.randperm(n, generator=g)[:k].sort()[0].to(x.device)
        mode = eng.mode
        try:
            eng.set_mode(1)                         # the exact-vote mode: the first pass's classifier tier depends on the mode
            fast = evaluate(idx, 1)
        finally:
            eng.set_mode(mode)
        top2 = fast.topk(2, dim=1)
        margin = top2.values[:, 0] - top2.values[:, 1]
        voted = (margin >= tau) & torch.isfinite(fast).all(1)
        vidx = idx[voted]
        rec = {'audited': int(k), 'voted_on_tier1': int(vidx.numel()), 'disagreements': [], 'max_leader_diff_error': 0.0,
               tau_key: tau, 'sigma': sigma}
        if spec:
            rec['loop'] = 'spec'
        if vidx.numel():
            mid = evaluate(vidx, 2)
            f = fast[voted]
            e = (f - mid).double()
            rec['max_leader_diff_error'] = float((e - e.gather(1, mid.argmax(1, keepdim=True))).abs().max())
            bad = (f.argmax(1) != mid.argmax(1)).nonzero().reshape(-1)
            rec['disagreements'] = [(int(vidx[j]), int(f[j].argmax()), int(mid[j].argmax()), float(margin[voted][j])) for j in bad.tolist()]
        self.audit_log.append(rec)
        if self.log is not None:
            self.log('audit%s: %d samples, %d voted on the 16-bit%s tier, %d disagree with the split-f16%s tier, largest leader-difference '
                     'error %.4g (%s %.4g)' % (' (spec loop)' if spec else '', rec['audited'], rec['voted_on_tier1'], unet, len(rec['disagreements']),
                                               unet, rec['max_leader_diff_error'], tau_key, tau))
        return rec

    @torch.no_grad()
    def certify(self, x: torch.Tensor, y: torch.Tensor, sigma: float = 0.25, n_0: int = 100, n: int = 100000,
                alpha: float = 0.001, batch_size: int = 64, audit: int = 0):
        y_pred, radius = -torch.ones_like(y), torch.zeros_like(y, dtype=torch.float32)
        for i in range(x.shape[0]):
            x_in = x[i]
            counts_0 = self.smooth_predict(x_in, num_sampling=n_0, sigma=sigma, batch_size=batch_size)
            c_A = counts_0.max(0, keepdim=True)[1].item()
            counts = self.smooth_predict(x_in, num_sampling=n, sigma=sigma, batch_size=batch_size)
            if audit > 0 and self._last is not None:       # opt-in: re-evaluate `audit` tier-1 voters of this example on a higher tier
                self.audit(x_in, audit)
            elif audit > 0 and not getattr(self, '_audit_warned', False):
                self._audit_warned = True
                (self.log or print)('audit requested but unavailable for this configuration (it needs the fused loop with device noise on an '
                                    'exact-vote engine: noise_source=%r, fused=%r): no "audit" entry will be written' % (self.noise_source, self._fused()))
            pa = self.lower_conf_bound(k=counts[c_A], n=n, alpha=alpha)
            if pa > 0.5:
                y_pred[i] = c_A
                radius[i] = sigma * norm.ppf(pa)
            else:
                y_pred[i] = -1
                radius[i] = 0
        return y_pred, radius,

    def compute_t_star(self, alpha_bar_star):
        Alpha_bar = self.denoiser.diffusion_hyperparams['Alpha_bar']
        return torch.abs(Alpha_bar - alpha_bar_star).min(0, keepdim=True)[1].item() + 1

    def lower_conf_bound(self, k, n, alpha=0.001):
        k = int(k)
        if k <= 0:
            return 0.0
        return float(_beta.ppf(alpha, k, n - k + 1))

    def certified_robust_correct(self, y_pred: torch.Tensor, y_target: torch.Tensor, r_c: torch.Tensor, r: float = 1.):
        correct = 0
        for i in range(len(y_pred)):
            if y_pred[i] == y_target[i] and r_c[i] >= r:
                correct += 1
        return correct
