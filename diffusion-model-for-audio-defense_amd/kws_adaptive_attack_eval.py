"""Adaptive-attack driver of the keyword-spotting task on the MI355X engine: the flags, data flow and printed metrics of the reference's
kws_adaptive_attack_eval.py, with the pieces of this package in place of the CUDA ones.

  python kws_adaptive_attack_eval.py --data_path <keyword dataset> --classifier_type vanilla --attack CW --max_iter_1 50
  python kws_adaptive_attack_eval.py --data_path <keyword dataset> --defense Diffusion --attack CW --t 1
  python kws_adaptive_attack_eval.py --data_path <keyword dataset> --clip_len 16000 --defense AS --attack FAKEBOB

The system is AcousticSystem(KWSModel on the engine, KWSMelSpectrogramDB on the same engine, defender): without a defender every forward
is one call of the engine (kws_wave_logits) and every CW gradient one more (kws_wave_vjp, `--grad_backend hip`), which compute only the
spectrogram frames the model reads.

Additions to the reference's flags:
  * `--classifier_path`: the checkpoint; by default the path the reference hard-codes for `--classifier_type`;
  * `--grad_backend {hip,torch}` (default hip): the engine's vector-Jacobian products, or the torch layers;
  * `--clip_len N` (default 0: every clip at its own length, as in the reference): with N > 0 every clip is padded or cut to N samples
    (FixAudioLength) and the engine is created for clips of N, which the defenses and the one-call queries need; N must be a multiple
    of 128.  Nothing is ever resampled;
  * `--max_clip_len N` (default 32000, a multiple of 128): the longest clip the native-length `--defense Diffusion` row takes; its engine
    is created for clips of N samples and a longer clip is refused;
  * the flags of the query-only drivers (`--nes_noise`, `--swarm_noise`, `--siren_loss`, `--seed`, `--defense_backend`).
At the native length `--attack CW` runs against `--defense None` and `--defense Diffusion`, at batch 1 as in the reference.  The native-length
Diffusion defender is, as in the reference, `RevDiffWave(args).model` — the DDPM DiffWave with reverse_timestep = args.t —, built with
any_length=True on an FP32 engine of `--max_clip_len` samples that also holds the keyword spotter: every clip is purified at its own
length on the exact-fp32 path (Engine.ddpm_purify_len), and `--grad_backend hip` differentiates through it with the engine's any-length
vector-Jacobian product.  With `--clip_len`: the attacks CW, FAKEBOB
and SirenAttack against the defenses None, Diffusion, AS, MS, DS, LPF and BPF.  Qin-I, Kenansville, Diffusion-Spec, FeCo and DefenseGAN
raise NotImplementedError naming the missing piece (Kenansville's FFT form runs on the 16000-sample clips of SC09, in
kenansville_attack_eval.py).
`run(args)` is importable so that tests can drive it without a subprocess; it returns the accuracy figures."""
import json
import os

import torch

import adaptive_attack_eval as white_box
import black_box_attack_eval as fakebob
import siren_attack_eval as siren

REFERENCE_CLASSIFIER_DIR = 'audio_models/RCNN_KWS/checkpoints'
REFERENCE_CLASSIFIER_FILE = {'vanilla': 'vanilla-best-acc-kws-attn_rcnn-n_mels=32.pth',
                             'advtr': 'advtr-best-robust-acc-kws-attn_rcnn-n_mels=32.pth'}
ATTACKS = ['CW', 'FAKEBOB', 'SirenAttack']
DEFENSES = ['None', 'Diffusion'] + list(white_box.BASELINE_DEFENSES)
_MISSING_ATTACK = {
    'Qin-I': 'the psychoacoustic masker at the clip lengths of this task (Engine.masking_step is built for 16000-sample clips behind the '
             'SC09 classifiers; the reference marks Qin-I "not used" here)',
    'Kenansville': 'the FFT attack of robustness_eval/black_box_attack.py on keyword clips (kenansville_attack_eval.py runs its FFT form on '
                   'the 16000-sample clips of SC09; the SSA form is not provided)',
}
_MISSING_DEFENSE = dict(white_box._MISSING_DEFENSE)
_MISSING_DEFENSE['Diffusion-Spec'] = ('a spectrogram purifier for [32 x T] spectrograms (the UNet of diffusion_models/improved_diffusion_sde.py is '
                                      'built for the 32 x 32 spectrograms of SC09)')


def build_parser():
    parser = white_box.build_parser()
    parser.description = __doc__
    parser.set_defaults(data_path='datasets/qualcomm_keyword_speech_dataset', classifier_type='advtr', classifier_path=None, max_iter_1=50,
                        dataload_workers_nums=0, batch_size=1)
    parser.add_argument('--clip_len', type=int, default=0, help='pad or cut every clip to N samples (a multiple of 128); 0: native length')
    parser.add_argument('--max_clip_len', type=int, default=32000,
                        help='native length, --defense Diffusion: the longest clip the purifier takes (a multiple of 128)')
    parser.add_argument('--nes_noise', choices=['device', 'torch'], default='device', help='FAKEBOB: the NES probe directions')
    parser.add_argument('--swarm_noise', choices=['device', 'numpy'], default='device', help='SirenAttack: the swarm')
    parser.add_argument('--siren_loss', choices=['reference', 'margin'], default='reference', help='SirenAttack: loss of the swarm')
    parser.add_argument('--seed', type=int, default=0, help='key of the device-side draws of FAKEBOB / SirenAttack')
    parser.add_argument('--defense_backend', choices=['hip', 'host'], default='hip',
                        help="a baseline defense on the engine's kernels, or on the host operators (torch / scipy)")
    return parser


def check_supported(args):
    """NotImplementedError for an attack / defense / option this driver does not run; ValueError for a --clip_len no engine takes."""
    if args.attack in _MISSING_ATTACK:
        raise NotImplementedError('--attack %s needs %s, which this package does not provide (supported: %s)'
                                  % (args.attack, _MISSING_ATTACK[args.attack], ', '.join(ATTACKS)))
    if args.attack not in ATTACKS:
        raise NotImplementedError('unknown attack: %s' % args.attack)
    if args.defense in _MISSING_DEFENSE:
        raise NotImplementedError('--defense %s needs %s, which this package does not provide (supported: %s)'
                                  % (args.defense, _MISSING_DEFENSE[args.defense], ', '.join(DEFENSES)))
    if args.defense not in DEFENSES:
        raise NotImplementedError('unknown defense: %s' % args.defense)
    if args.max_iter_2 > 0:
        raise NotImplementedError('--max_iter_2 > 0 runs AudioAttack stage 2 (Qin-I), which needs %s' % _MISSING_ATTACK['Qin-I'])
    if args.clip_len < 0 or args.clip_len % 128:
        raise ValueError('--clip_len %d: the engine takes clips whose length is a multiple of 128 (0: the native length)' % args.clip_len)
    if args.clip_len == 0:
        if args.attack != 'CW' or args.defense not in ('None', 'Diffusion'):
            raise NotImplementedError('--attack %s --defense %s needs clips of one length: pass --clip_len N (the defenses and the one-call '
                                      'queries run at the clip length the engine was created for); at the native length only --attack CW '
                                      '--defense None runs' % (args.attack, args.defense))
        if args.defense == 'Diffusion' and (args.max_clip_len < 128 or args.max_clip_len % 128):
            raise ValueError('--max_clip_len %d: the purifier\'s engine takes a clip length that is a positive multiple of 128' % args.max_clip_len)
        if args.batch_size != 1:
            raise NotImplementedError('--batch_size %d at the native length: clips of different lengths do not stack, pass --clip_len N '
                                      '(the reference runs this task at batch 1)' % args.batch_size)
    elif not 800 <= args.clip_len <= 128799:
        raise ValueError('--clip_len %d: the keyword spotter on the engine serves 800 .. 128799 samples' % args.clip_len)
    if args.clip_len not in (0, 16000) and args.defense == 'Diffusion':
        raise NotImplementedError('--defense Diffusion with --clip_len %d: the DiffWave purifier runs on the shared engine, which is created '
                                  'for 16000-sample clips; pass --clip_len 16000' % args.clip_len)


def classifier_path(args):
    return args.classifier_path or os.path.join(REFERENCE_CLASSIFIER_DIR, REFERENCE_CLASSIFIER_FILE[args.classifier_type])


def build_system(args, classifier=None, defender=None, engine=None):
    """AcousticSystem of the driver's flags: KWSModel and its mel front-end on one engine (`engine`, or the shared one for --defense
    Diffusion at --clip_len 16000, or one created for --clip_len, or the FP32 engine of --max_clip_len samples of the native-length
    Diffusion row), and the defender.  `classifier` / `defender` may be passed ready-made (tests)."""
    from acoustic_system import AcousticSystem
    from audio_models.RCNN_KWS.model import load_checkpoint
    from dmad_hip import engine as E
    from dmad_hip.transforms import KWSMelSpectrogramDB
    if classifier is None:
        classifier = load_checkpoint(classifier_path(args))
    classifier.cuda().eval()
    native_diffusion = args.clip_len == 0 and args.defense == 'Diffusion'
    if native_diffusion and defender is None:
        # as in the reference: the DDPM DiffWave inside RevDiffWave, here on one FP32 engine with the keyword spotter, any length <= N
        from diffusion_models.diffwave_sde import RevDiffWave
        if engine is None:
            with open(args.ddpm_config) as f:
                wavenet_config = json.load(f)['wavenet_config']
            engine = E.Engine(wavenet_config, clip_len=args.max_clip_len, max_batch=1, precision=E.FP32, with_classifier=False)
        defender = RevDiffWave(args, engine=engine, any_length=True, grad_backend=args.grad_backend).model
    if native_diffusion and engine is None:
        engine = getattr(defender, 'engine', None)
    if 'engine' not in classifier.__dict__:
        if engine is None and args.defense != 'Diffusion':
            engine = E.Engine(clip_len=args.clip_len or 16000, max_batch=int(os.environ.get('DMAD_MAX_BATCH', '64')), precision=E.FP32,
                              with_wavenet=False, with_classifier=False)
        classifier.use_engine(engine)
    classifier.grad_backend = args.grad_backend
    eng = classifier.__dict__['engine']
    wave2spect = KWSMelSpectrogramDB(eng, grad_backend=args.grad_backend)
    if args.defense == 'None':
        defender = None
    elif native_diffusion:
        defender = MaxClipLen(defender, args.max_clip_len)
    elif args.defense == 'Diffusion':
        if defender is None:
            from diffusion_models.diffwave_sde import RevDiffWave
            defender = RevDiffWave(args, **({} if args.score_grad is None else {'score_grad': args.score_grad}))
    elif defender is None:
        from baseline_defense_eval import build_defender
        defender = build_defender(args, eng)
    return AcousticSystem(classifier=classifier, transform=wave2spect, defender=defender, defense_type='wave'), classifier


class MaxClipLen(torch.nn.Module):
    """The native-length Diffusion defender behind the driver's length check: a clip longer than --max_clip_len is refused by name of
    the flag, instead of by the engine's shape error."""

    def __init__(self, purifier, max_clip_len):
        super().__init__()
        self.purifier, self.max_clip_len = purifier, int(max_clip_len)

    def _get_name(self):                      # the evaluation loop logs the defender's name: the purifier's, as in the reference
        return self.purifier._get_name()

    def forward(self, x):
        if x.shape[-1] > self.max_clip_len:
            raise ValueError('a clip of %d samples is longer than --max_clip_len %d: pass a larger --max_clip_len (a multiple of 128)'
                             % (x.shape[-1], self.max_clip_len))
        return self.purifier(x)


def build_dataset(args):
    from datasets.qualcomm_kws_dataset import FixAudioLength, LoadAudio, QualcommKeywordSpottingDataset
    ts = [LoadAudio()] + ([FixAudioLength(args.clip_len / 16000.0)] if args.clip_len else [])
    return QualcommKeywordSpottingDataset(folder=args.data_path, usage='Test', transform=white_box._Compose(ts))


def run(args, classifier=None, defender=None, log=print, engine=None, **attack_overrides):
    """The reference's evaluation loop.  Returns {'total', 'clean_acc', 'denoised_acc', 'robust_acc'} (accuracies in percent)."""
    check_supported(args)
    torch.cuda.set_device(args.gpu)
    AS_MODEL, classifier = build_system(args, classifier, defender, engine)
    log('classifier type: {}'.format(args.classifier_type))
    if args.attack == 'CW':
        if attack_overrides:
            raise TypeError('the CW attacker takes its constants from the flags, not from overrides: %s' % sorted(attack_overrides))
        make_attacker = white_box.attacker_factory(args, AS_MODEL, log)
    else:
        make_attacker = (fakebob if args.attack == 'FAKEBOB' else siren).attacker_factory(args, AS_MODEL, log, **attack_overrides)
    return white_box.evaluate(args, AS_MODEL, classifier, make_attacker, log, test_dataset=build_dataset(args))


if __name__ == '__main__':
    run(build_parser().parse_args())
