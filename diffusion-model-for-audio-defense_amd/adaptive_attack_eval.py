"""White-box adaptive-attack driver on the MI355X engine: the flags, data flow and printed metrics of the reference's
adaptive_attack_eval.py, with the pieces of this package in place of the CUDA ones.

  python adaptive_attack_eval.py --data_path <SC09 test folder> --defense Diffusion --t 2 --eps 65 --max_iter_1 10

What it runs: the CW (sign-gradient, `robustness_eval.white_box_attack.AudioAttack` stage 1) attack against
AcousticSystem(classifier, MelSpectrogramDB, defender) with the defenses
  * None            classifier and mel front-end only;
  * Diffusion       RevDiffWave (the reverse VP-SDE on the waveform, diffusion_models/diffwave_sde.py);
  * Diffusion-Spec  RevImprovedDiffusion (the reverse VP-SDE on the spectrogram, diffusion_models/improved_diffusion_sde.py).
Every other attack (Qin-I, Kenansville, FAKEBOB, SirenAttack) and defense (AS, MS, DS, LPF, BPF, FeCo, DefenseGAN) raises
NotImplementedError naming the piece this package does not have, or the driver that runs it (Qin-I and `--max_iter_2` > 0:
imperceptible_attack_eval.py; FAKEBOB, SirenAttack and Kenansville (FFT form): black_box_attack_eval.py, siren_attack_eval.py and
kenansville_attack_eval.py; the baseline defenses AS, MS,
DS, LPF, BPF: baseline_defense_eval.py).

Additions to the reference's flags:
  * `--classifier_path`: the classifier checkpoint; its default is the path the reference hard-codes (it overrides
    `--classifier_model` / `--classifier_type`, which are kept for compatibility and otherwise unused, as in the reference);
  * `--grad_backend {hip,torch}` (default hip): the gradient of the classifier (ResNeXt29, VGG19_bn, WideResNet-28-10, DenseNet-BC-100-12 or M5) and of the mel
    front-end — the engine's vector-Jacobian products, or the torch layers.  An M5 checkpoint (`M5Net.M5`) classifies the raw
    waveform: the system is AcousticSystem(classifier, transform=None, ...) as in the reference, and `--defense Diffusion-Spec` is refused;
  * `--score_grad`: passed to the SDE purifiers (default: their module defaults, 'none' for RevDiffWave, 'hip' for
    RevImprovedDiffusion).
`--save_path` writes the clean / purified / adversarial waveforms as 16-bit WAV files (standard library only); the reference's
spectrogram images of `--defense Diffusion-Spec` need a plotting library and are refused.  The reference writes the unpurified
adversarial clip under the `_adv_purified` name; this driver writes the purified one there.
`run(args)` is importable so that tests can drive it without a subprocess; it returns the accuracy figures."""
import argparse
import os
import wave

import torch
from torch.utils.data import DataLoader

REFERENCE_CLASSIFIER_PATH = ('audio_models/ConvNets_SpeechCommands/checkpoints/jacobian_reg_resnext29_8_64_sgd_plateau_bs96_lr1.0e-02_wd1.0e-02/'
                             'reg=1e-08-best-robust-acc.pth')
ATTACKS = ['CW', 'Qin-I', 'Kenansville', 'FAKEBOB', 'SirenAttack']
DEFENSES = ['Diffusion', 'Diffusion-Spec', 'AS', 'MS', 'DS', 'LPF', 'BPF', 'FeCo', 'DefenseGAN', 'None']
_MISSING_ATTACK = {}
# query-only attacks run by a driver of their own (Kenansville: its FFT form; the SSA form is not provided)
_OTHER_DRIVER = {'FAKEBOB': 'black_box_attack_eval.py', 'SirenAttack': 'siren_attack_eval.py', 'Kenansville': 'kenansville_attack_eval.py'}
QIN_DRIVER = 'imperceptible_attack_eval.py'       # Qin-I (AudioAttack stage 2, max_iter_2 > 0)
BASELINE_DEFENSES = ['AS', 'MS', 'DS', 'LPF', 'BPF']                # transforms/time_defense.py, transforms/frequency_defense.py
_MISSING_DEFENSE = {
    'FeCo': 'the feature-compression defense (transforms/feature_defense.py)',
    'DefenseGAN': 'the DefenseGAN purifier (gan_models/DefenseGAN.py)',
}


class _Compose:
    def __init__(self, ts):
        self.ts = ts

    def __call__(self, x):
        for t in self.ts:
            x = t(x)
        return x


def build_parser():
    parser = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    # SC09 classifier arguments
    parser.add_argument("--data_path", default='datasets/speech_commands/test')
    parser.add_argument("--classifier_model", type=str, choices=['resnext29_8_64', 'vgg19_bn', 'densenet_bc_100_12', 'wideresnet28_10', 'm5'],
                        default='resnext29_8_64')
    parser.add_argument("--classifier_type", type=str, choices=['advtr', 'vanilla'], default='vanilla')
    parser.add_argument("--classifier_input", choices=['mel32'], default='mel32', help='input of NN')
    parser.add_argument("--num_per_class", type=int, default=10)
    parser.add_argument("--classifier_path", default=REFERENCE_CLASSIFIER_PATH,
                        help='classifier checkpoint (default: the path the reference driver hard-codes)')
    # DiffWave-VPSDE arguments
    parser.add_argument('--ddpm_config', type=str, default='configs/config.json', help='JSON file for configuration')
    parser.add_argument('--ddpm_path', type=str, default='diffusion_models/DiffWave_Unconditional/exp/ch256_T200_betaT0.02/logs/checkpoint/1000000.pkl')
    parser.add_argument('--sample_step', type=int, default=1, help='Total sampling steps')
    parser.add_argument('--t', type=int, default=1, help='Sampling noise scale')
    parser.add_argument('--t_delta', type=int, default=15, help='Perturbation range of sampling noise scale')
    parser.add_argument('--rand_t', action='store_true', default=False, help='Decide if randomize sampling noise scale')
    parser.add_argument('--diffusion_type', type=str, default='ddpm', help='[ddpm, sde]')
    parser.add_argument('--score_type', type=str, default='guided_diffusion', help='[guided_diffusion, score_sde, ddpm]')
    parser.add_argument('--use_bm', action='store_true', default=False, help='whether to use brownian motion')
    parser.add_argument('--score_grad', choices=['none', 'hip', 'torch'], default=None,
                        help='gradient of the SDE purifiers (default: the module default of RevDiffWave / RevImprovedDiffusion)')
    # attack arguments
    parser.add_argument('--attack', type=str, choices=ATTACKS, default='CW')
    parser.add_argument('--defense', type=str, choices=DEFENSES, default='None')
    parser.add_argument('--bound_norm', type=str, choices=['linf', 'l2'], default='linf')
    parser.add_argument('--eps', type=int, default=65)
    parser.add_argument('--max_iter_1', type=int, default=10)
    parser.add_argument('--max_iter_2', type=int, default=0)
    parser.add_argument('--eot_attack_size', type=int, default=1)
    parser.add_argument('--eot_defense_size', type=int, default=1)
    parser.add_argument('--verbose', type=int, default=1)
    parser.add_argument('--grad_backend', choices=['hip', 'torch'], default='hip',
                        help='gradient of the classifier (ResNeXt29, VGG19_bn, WideResNet-28-10, DenseNet-BC-100-12, M5) and of the mel front-end: the engine VJPs or the torch layers')
    # device arguments
    parser.add_argument("--dataload_workers_nums", type=int, default=8, help='number of workers for dataloader')
    parser.add_argument("--batch_size", type=int, default=20, help='batch size')
    parser.add_argument('--gpu', type=int, default=0)
    # file saving arguments
    parser.add_argument('--save_path', default=None)
    return parser


def check_supported(args):
    """NotImplementedError for an attack / defense / option this package does not provide."""
    if args.attack in _OTHER_DRIVER:
        raise NotImplementedError('--attack %s is a query-only attack: %s runs it, this white-box driver does not'
                                  % (args.attack, _OTHER_DRIVER[args.attack]))
    if args.attack == 'Qin-I':
        raise NotImplementedError('--attack Qin-I is the two-stage imperceptible attack: %s runs it, this driver runs stage 1 (CW) only'
                                  % QIN_DRIVER)
    if args.attack in _MISSING_ATTACK:
        raise NotImplementedError('--attack %s needs %s, which this package does not provide (supported: CW)'
                                  % (args.attack, _MISSING_ATTACK[args.attack]))
    if args.attack != 'CW':
        raise NotImplementedError('unknown attack: %s' % args.attack)
    check_defense(args)
    if args.max_iter_2 > 0:
        raise NotImplementedError('--max_iter_2 > 0 runs AudioAttack stage 2 (Qin-I): %s runs it, this driver runs stage 1 only' % QIN_DRIVER)


def check_defense(args):
    """The part of check_supported that does not depend on the attack (shared with black_box_attack_eval.py): the defense and --save_path."""
    if args.defense in BASELINE_DEFENSES:
        raise NotImplementedError('--defense %s is a baseline waveform defense: baseline_defense_eval.py runs it (with --attack CW, FAKEBOB '
                                  'or SirenAttack), this driver does not (supported: None, Diffusion, Diffusion-Spec)' % args.defense)
    if args.defense in _MISSING_DEFENSE:
        raise NotImplementedError('--defense %s needs %s, which this package does not provide (supported: None, Diffusion, Diffusion-Spec)'
                                  % (args.defense, _MISSING_DEFENSE[args.defense]))
    if args.defense not in ('None', 'Diffusion', 'Diffusion-Spec'):
        raise NotImplementedError('unknown defense: %s' % args.defense)
    if args.save_path is not None and args.defense == 'Diffusion-Spec':
        raise NotImplementedError('--save_path with --defense Diffusion-Spec writes spectrogram images, which needs a plotting library '
                                  'this package does not use')


def _save_wav(x, path, name):
    pcm = (x.detach().reshape(-1).clamp(-1, 1).cpu().numpy() * 32767.0).round().astype('<i2')
    with wave.open(os.path.join(path, name), 'wb') as w:
        w.setnchannels(1)
        w.setsampwidth(2)
        w.setframerate(16000)
        w.writeframes(pcm.tobytes())


def build_system(args, classifier=None, defender=None):
    """AcousticSystem of the driver's flags.  `classifier` / `defender` may be passed ready-made (tests, synthetic weights)."""
    from acoustic_system import AcousticSystem
    check_defense(args)
    classifier, wave2spect = build_front(args, classifier)
    kw = {} if args.score_grad is None else {'score_grad': args.score_grad}
    if args.defense == 'None':
        return AcousticSystem(classifier=classifier, transform=wave2spect, defender=None), classifier
    if args.defense == 'Diffusion':
        if defender is None:
            from diffusion_models.diffwave_sde import RevDiffWave
            defender = RevDiffWave(args, **kw)
        elif args.score_grad is not None:
            defender.score_grad = args.score_grad
        system = AcousticSystem(classifier=classifier, transform=wave2spect, defender=defender, defense_type='wave')
    else:
        if defender is None:
            from diffusion_models.improved_diffusion_sde import RevImprovedDiffusion
            defender = RevImprovedDiffusion(args, **kw)
        elif args.score_grad is not None:
            defender.score_grad = args.score_grad
        system = AcousticSystem(classifier=classifier, transform=wave2spect, defender=defender, defense_type='spec')
    return system, classifier


def _is_m5(classifier):
    from audio_models.M5.M5Net import is_m5
    return is_m5(classifier)


def check_classifier_defense(args, classifier):
    """NotImplementedError for a defense the loaded classifier cannot stand behind."""
    if args.defense == 'Diffusion-Spec' and _is_m5(classifier):
        raise NotImplementedError('--defense Diffusion-Spec purifies the mel spectrogram, and the M5 checkpoint classifies the raw waveform '
                                  '(AcousticSystem(classifier, transform=None, ...)): a spectrogram purifier cannot stand in front of a '
                                  'waveform classifier (supported with M5: None, Diffusion, and the baseline defenses of baseline_defense_eval.py)')


def build_front(args, classifier=None):
    """The classifier of the driver's flags on its engine, and the mel front-end on the same engine (shared with baseline_defense_eval.py);
    for an M5 checkpoint the classifier on its engine (M5.use_engine) and None: it has no front-end."""
    from audio_models.ConvNets_SpeechCommands.create_model import create_model
    from dmad_hip.transforms import MelSpectrogramDB
    if classifier is None:
        classifier = create_model(args.classifier_path)
    check_classifier_defense(args, classifier)
    classifier.cuda()
    if _is_m5(classifier):               # reference l.121-122, 169-170: M5 takes the raw audio, AcousticSystem(classifier, transform=None, ...)
        classifier.eval()
        if 'engine' not in classifier.__dict__:
            classifier.use_engine()
        classifier.grad_backend = args.grad_backend
        return classifier, None
    if hasattr(classifier, 'bind_engine') and 'engine' not in classifier.__dict__:
        classifier.bind_engine()
    if 'torch' in getattr(classifier, 'GRAD_BACKENDS', ()) and 'hip' in classifier.GRAD_BACKENDS:    # ResNeXt29, VGG19_bn, WideResNet-28-10 and DenseNet-BC-100-12
        classifier.grad_backend = args.grad_backend
    return classifier, MelSpectrogramDB(classifier.__dict__.get('engine'), grad_backend=args.grad_backend)


def run(args, classifier=None, defender=None, log=print):
    """The reference's evaluation loop.  Returns {'total', 'clean_acc', 'denoised_acc', 'robust_acc'} (accuracies in percent)."""
    from robustness_eval.white_box_attack import AudioAttack
    check_supported(args)
    torch.cuda.set_device(args.gpu)
    AS_MODEL, classifier = build_system(args, classifier, defender)
    return evaluate(args, AS_MODEL, classifier, attacker_factory(args, AS_MODEL, log), log)


def attacker_factory(args, AS_MODEL, log=print):
    """make_attacker() of evaluate(): the CW attacker of the driver's flags (shared with baseline_defense_eval.py)."""
    from robustness_eval.white_box_attack import AudioAttack

    def make_attacker():
        Attacker = AudioAttack(model=AS_MODEL, eps=args.eps, norm=args.bound_norm, max_iter_1=args.max_iter_1, max_iter_2=0,
                               learning_rate_1=args.eps / 5 if args.bound_norm == 'linf' else args.eps / 50,
                               eot_attack_size=args.eot_attack_size, eot_defense_size=args.eot_defense_size, verbose=args.verbose)
        log('attack: {} with {}_eps={} & iter={} & eot={}-{}'.format(args.attack, args.bound_norm, args.eps, args.max_iter_1,
                                                                    args.eot_attack_size, args.eot_defense_size))
        return Attacker
    return make_attacker


def evaluate(args, AS_MODEL, classifier, make_attacker, log=print, test_dataset=None):
    """The evaluation loop the attack drivers share (reference l.234-370): clean, purified-clean and attacked accuracy over the test folder
    (`test_dataset`: another dataset of {'samples', 'target'} items, as kws_adaptive_attack_eval.py passes).
    `make_attacker()` is called after the model lines are logged and returns an object with generate(x=, y=, targeted=) -> (x_adv, success),
    success a list per clip or the (stage 1, stage 2) pair of AudioAttack."""
    from datasets.sc_dataset import SC09Dataset
    from transforms import FixAudioLength, LoadAudio
    AS_MODEL.eval()
    if test_dataset is None:
        test_dataset = SC09Dataset(folder=args.data_path, transform=_Compose([LoadAudio(), FixAudioLength()]), num_per_class=args.num_per_class)
    test_dataloader = DataLoader(test_dataset, batch_size=args.batch_size, sampler=None, shuffle=False, pin_memory=True,
                                 num_workers=args.dataload_workers_nums)
    log('classifier model: {}'.format(classifier._get_name()))
    log('defense: {}'.format(args.defense if AS_MODEL.defender is None else '{} with t={}'.format(AS_MODEL.defender._get_name(), args.t)))
    Attacker = make_attacker()
    correct_orig = correct_orig_denoised = correct_adv_1 = total = 0
    acc_orig = acc_orig_denoised = acc_adv_1 = 0.0
    for batch in test_dataloader:
        waveforms = torch.unsqueeze(batch['samples'], 1).cuda()
        targets = batch['target'].cuda()
        with torch.no_grad():
            pred_clean = AS_MODEL(waveforms, False).max(1, keepdim=True)[1].squeeze()
            if AS_MODEL.defense_type == 'wave':
                waveforms_defended = waveforms if AS_MODEL.defender is None else AS_MODEL.defender(waveforms)
                pred_defended = AS_MODEL(waveforms_defended, False).max(1, keepdim=True)[1].squeeze()
            else:
                spectrogram = AS_MODEL.transform(waveforms)
                spectrogram_defended = AS_MODEL.defender(spectrogram)
                pred_defended = AS_MODEL.classifier(spectrogram_defended).max(1, keepdim=True)[1].squeeze()
        waveforms_adv, attack_success = Attacker.generate(x=waveforms, y=targets, targeted=False)
        if args.save_path is not None:
            with torch.no_grad():
                adv_defended = waveforms_adv if AS_MODEL.defender is None else AS_MODEL.defender(waveforms_adv)
            clean_path, adv_path = os.path.join(args.save_path, 'clean'), os.path.join(args.save_path, 'adv')
            os.makedirs(clean_path, exist_ok=True)
            os.makedirs(adv_path, exist_ok=True)
            for i in range(waveforms.shape[0]):
                audio_id, y = str(total + i).zfill(3), targets[i].item()
                _save_wav(waveforms[i], clean_path, '{}_{}_clean.wav'.format(audio_id, y))
                _save_wav(waveforms_defended[i], clean_path, '{}_{}_clean_purified.wav'.format(audio_id, y))
                _save_wav(waveforms_adv[i], adv_path, '{}_{}_adv.wav'.format(audio_id, y))
                _save_wav(adv_defended[i], adv_path, '{}_{}_adv_purified.wav'.format(audio_id, y))
        first_stage = attack_success[0] if isinstance(attack_success, tuple) else attack_success
        total += waveforms.shape[0]
        correct_orig += (pred_clean == targets).sum().item()
        correct_orig_denoised += (pred_defended == targets).sum().item()
        correct_adv_1 += waveforms.shape[0] - int(torch.tensor(first_stage).sum().item())
        acc_orig = correct_orig / total * 100
        acc_orig_denoised = correct_orig_denoised / total * 100
        acc_adv_1 = correct_adv_1 / total * 100
        log('{} / {}: orig clean acc {:.4f}%, denoised clean acc {:.4f}%, {} robust acc {:.4f}%'.format(
            total, len(test_dataset), acc_orig, acc_orig_denoised, args.attack, acc_adv_1))
    log('on {} test examples: '.format(total))
    log('original clean test accuracy: {:.4f}%'.format(acc_orig))
    log('denoised clean test accuracy: {:.4f}%'.format(acc_orig_denoised))
    log('CW robust test accuracy: {:.4f}%'.format(acc_adv_1))           # the reference prints this label for every attack
    return {'total': total, 'clean_acc': acc_orig, 'denoised_acc': acc_orig_denoised, 'robust_acc': acc_adv_1}


if __name__ == '__main__':
    run(build_parser().parse_args())
