"""Host mirror of the reference's acoustic_system.AcousticSystem (acoustic_system.py:3-51):
defender (waveform purifier) -> transform (waveform -> spectrogram) -> classifier, with the same
constructor, attributes and error behaviour.  The stages themselves are the HIP-backed modules of this
package (DiffWave, MelSpectrogramDB, VGG) or any callables the caller passes.

`query(x, repeats)` is the batched entry of the gradient-free attack drivers (EOT / NES): every clip evaluated
`repeats` times with fresh purification noise.  When the three stages are this package's HIP stages on one engine it is
ONE C-ABI call — dmad_query_logits for defense_type 'wave' (repeat -> DDPM purify -> mel dB -> classifier -> arg-max),
dmad_defense_query_logits for a baseline waveform defense (TimeDomainDefense / FreqDomainDefense on backend 'hip'),
dmad_spec_query_logits for 'spec' (repeat -> mel dB -> spec-domain purifier -> classifier -> arg-max).  With transform None and an
M5 that use_engine() put on the engine the 'wave' chains are dmad_m5_query_logits / dmad_m5_defense_query_logits (the same rows and
Philox keys, M5 in the place of mel dB -> classifier).  A KWSModel that use_engine() put on the engine behind the keyword spotter's own mel front-end
on that engine (dmad_hip.transforms.KWSMelSpectrogramDB, or the shims' MelSpectrogram(sample_rate=16000, n_mels=32) + AmplitudeToDB pair)
is the third family: forward() itself is one call there (kws_wave_logits, or autograd.KWSWaveHIP on the gradient branch with grad_backend
'hip'), and the 'wave' chains are dmad_kws_query_logits / dmad_kws_defense_query_logits, which need clips of the engine's clip_len (without
a defender any length runs, as kws_wave_logits on the repeated rows).  Otherwise it loops over forward()."""
import torch


class AcousticSystem(torch.nn.Module):

    def __init__(self, classifier: torch.nn.Module, transform, defender: torch.nn.Module = None, defense_type: str = 'wave'):
        super().__init__()
        self.classifier = classifier
        self.transform = transform
        self.defender = defender
        self.defense_type = defense_type
        if self.defense_type not in ['wave', 'spec']:
            raise NotImplementedError('argument defense_type should be \'wave\' or \'spec\'!')

    @staticmethod
    def _rescale(x):
        # int16-range input is rescaled to [-1, 1] (acoustic_system.py:29-30)
        if 0.9 * x.max() > 1 and 0.9 * x.min() < -1:
            x = x / (2 ** 15)
        return x

    def forward(self, x, defend=True):
        x = self._rescale(x)
        use_defender = defend == True and self.defender is not None   # noqa: E712 (reference semantics)
        output = self.defender(x) if (use_defender and self.defense_type == 'wave') else x
        eng = self._kws_engine() if output.is_cuda and not (use_defender and self.defense_type == 'spec') else None
        if eng is not None:                                           # KWSModel behind its own front-end, both on one engine: one call
            if not (torch.is_grad_enabled() and output.requires_grad):
                return eng.kws_wave_logits(output)
            if self.classifier.grad_backend == 'hip' and getattr(self.transform, 'grad_backend', 'hip') == 'hip':
                from dmad_hip.autograd import kws_wave_hip
                return kws_wave_hip(eng, output)
        if self.transform is not None:
            output = self.transform(output)
        if use_defender and self.defense_type == 'spec':
            output = self.defender(output)
        return self.classifier(output)

    # ------------------------------------------------------------------------------------------------------------
    @staticmethod
    def _stages(tr):
        """the `_dmad_stage` names of a Compose (`.transforms`) or an nn.Sequential, and the stages themselves"""
        ts = getattr(tr, 'transforms', None)
        if ts is None and isinstance(tr, torch.nn.Sequential):
            ts = list(tr.children())
        ts = list(ts or [])
        return [getattr(t, '_dmad_stage', None) for t in ts], ts

    def _kws_engine(self):
        """The engine of a KWSModel in eval mode whose transform is the keyword spotter's mel front-end on the same engine, or None."""
        from audio_models.RCNN_KWS.model import is_kws
        cls, tr = self.classifier, self.transform
        eng = getattr(cls, 'engine', None) if 'engine' in getattr(cls, '__dict__', {}) else None
        if eng is None or tr is None or not is_kws(cls) or cls.training:
            return None
        if getattr(tr, '_dmad_stage', None) == 'kws_mel_db':          # dmad_hip.transforms.KWSMelSpectrogramDB
            return eng if tr.engine is eng else None
        names, ts = self._stages(tr)
        return eng if names == ['kws_mel_power', 'power_to_db'] and getattr(ts[0], 'engine', None) is eng else None

    def _engine_chain(self, defend, L=None):
        """The engine that can run this system as one dmad_query_logits call, with the sampler id, or (None, 0).  L: the clip length of
        the query, which the KWS chains with a defender need to be the engine's."""
        from dmad_hip.transforms import MelSpectrogramDB
        cls, tr, den = self.classifier, self.transform, self.defender
        eng = getattr(cls, 'engine', None) if 'engine' in getattr(cls, '__dict__', {}) else None
        if eng is None:
            return None, 0
        if tr is None:                                                # waveform classifier: an M5 on the engine (M5.use_engine)
            from audio_models.M5.M5Net import is_m5
            if not (is_m5(cls) and eng.has_m5 and not cls.training and self.defense_type == 'wave'):
                return None, 0
            return self._wave_sampler(eng, defend)                    # the same samplers; query() calls the engine's m5_* pair for them
        from audio_models.RCNN_KWS.model import is_kws
        if is_kws(cls):                                               # a KWSModel's `engine` is not a spectrogram-classifier binding:
            if self._kws_engine() is not eng or self.defense_type != 'wave':      # only behind its own front-end is it a one-call chain
                return None, 0
            eng, sampler = self._wave_sampler(eng, defend)
            return (None, 0) if (sampler and L != eng.L) else (eng, sampler)      # the purifier and the defenses run at clip_len only
        if not eng.has_classifier:
            return None, 0
        mel = isinstance(tr, MelSpectrogramDB) and tr.engine is eng
        if not mel:
            mel = [getattr(t, '_dmad_stage', None) for t in getattr(tr, 'transforms', [])] == ['mel_power', 'power_to_db']
        if not mel:
            return None, 0
        if self.defense_type == 'spec' and defend == True and den is not None:   # noqa: E712  sampler 3: the spec-domain chain (dmad_spec_query_logits)
            from diffusion_models.improved_diffusion_ddpm import SpecPurifier
            return (eng, 3) if (type(den) is SpecPurifier and den.engine is eng) else (None, 0)
        return self._wave_sampler(eng, defend)

    def _wave_sampler(self, eng, defend):
        """(eng, sampler) of the waveform defender in front of the engine's classifier stage: 0 none, 1 DiffWave on device noise, 4 a
        baseline waveform defense on backend 'hip'; (None, 0) for anything else."""
        from diffusion_models.diffwave_ddpm import DiffWave
        den = self.defender
        if not (defend == True and den is not None):                  # noqa: E712
            return eng, 0
        if type(den) is DiffWave and den.noise_source == 'device' and den.engine is eng and eng.has_wavenet:
            return eng, 1
        from transforms.time_defense import TimeDomainDefense
        from transforms.frequency_defense import FreqDomainDefense
        if ((type(den) is TimeDomainDefense and den.defense_type in ('AS', 'MS')) or
                (type(den) is FreqDomainDefense and den.defense_type in ('DS', 'LPF', 'BPF'))) and den.backend == 'hip' and den.engine is eng:
            return eng, 4                                             # sampler 4: a baseline waveform defense (dmad_defense_query_logits)
        return None, 0

    @torch.no_grad()
    def query(self, x, repeats: int, defend=True, per_call: int = None):
        """x [B,1,L] -> (logits [repeats, B, C], decisions int64 [repeats, B]); repeat r of clip b is row (r, b), the
        order of `model(x.repeat(repeats, 1, 1))` (robustness_eval/_EOT.py:36-40).  Without a one-engine chain (other
        stages, or a purifier on the reference's CPU noise stream) the system is called the way the reference's EOT calls
        it: `repeats / per_call` forward passes over x.repeat(per_call, 1, 1), which also consumes the CPU generator in
        the reference's order."""
        x = self._rescale(x)
        B = x.shape[0]
        eng, sampler = self._engine_chain(defend, x.shape[-1])
        if eng is not None and x.is_cuda:
            # a chain without a transform is an M5 on the engine: the same rows and keys, M5 in the place of mel dB -> classifier;
            # a chain that _kws_engine() recognises is a KWSModel behind its own mel front-end in that place
            pre = 'm5_' if self.transform is None else ('kws_' if self._kws_engine() is eng else '')
            if pre == 'kws_' and sampler == 0:                        # no purifier, no defense: the rows at any length, in one call
                logits, dec = eng.kws_wave_logits(x.repeat(repeats, 1, 1), want_decisions=True)
                return logits.view(repeats, B, -1), dec.view(repeats, B).long()
            if sampler == 1:
                den = self.defender
                from diffusion_models.diffwave_ddpm import fixed_length_only
                fixed_length_only(den.model, x, 'the one-call query (dmad_query_logits)')
                ts, c_a, c_b, c_eps, c_div, c_sig = den.purify_coefficients()
                logits, dec = getattr(eng, pre + 'query_logits')(x, repeats, 1, ts, c_a, c_b, c_eps, c_div, c_sig, seed=den.seed, sample0=den._draws)
                den._draws += repeats * B
            elif sampler == 3:
                from diffusion_models.Improved_Diffusion_Unconditional.improved_diffusion.sc09_spectrogram_dataset import MEL_LOWER_BOUND, MEL_UPPER_BOUND
                den = self.defender
                logits, dec = eng.spec_query_logits(x, repeats, *den.purifier.purify_coefficients(), MEL_LOWER_BOUND, MEL_UPPER_BOUND,
                                                    seed=den.seed, sample0=den._draws)
                den._draws += repeats * B
            elif sampler == 4:
                den = self.defender
                logits, dec = getattr(eng, pre + 'defense_query_logits')(x, repeats, den.engine_defense(x))
            else:
                logits, dec = getattr(eng, pre + 'query_logits')(x, repeats, 0)
            return logits.view(repeats, B, -1), dec.view(repeats, B).long()
        per_call = per_call or repeats
        assert repeats % per_call == 0
        logits = torch.cat([self.forward(x.repeat(per_call, 1, 1), defend).view(per_call, B, -1) for _ in range(repeats // per_call)])
        return logits, logits.argmax(-1)
