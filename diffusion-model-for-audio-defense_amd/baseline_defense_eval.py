"""Baseline-defense driver on the MI355X engine: the transformation defenses the diffusion purifiers are compared against, under the
three attacks this package runs.

  python baseline_defense_eval.py --data_path <SC09 test folder> --attack CW --defense BPF
  python baseline_defense_eval.py --data_path <SC09 test folder> --attack FAKEBOB --defense AS

  --attack   CW | FAKEBOB | SirenAttack           the attackers of adaptive_attack_eval.py, black_box_attack_eval.py, siren_attack_eval.py
  --defense  AS | MS (transforms/time_defense.py)  DS | LPF | BPF (transforms/frequency_defense.py)

The flags and constants are the reference driver's (adaptive_attack_eval.py there offers these defenses next to the diffusion ones), the
evaluation loop is adaptive_attack_eval.evaluate, and the attacker is built by the driver that owns the attack.  Under CW the gradient of
the classifier (ResNeXt29 or VGG19_bn) and of the mel front-end follows adaptive_attack_eval's `--grad_backend` (default hip: the engine's
vector-Jacobian products).  One flag is added:
  * `--defense_backend {hip,host}` (default hip): the engine's kernels (dmad_wave_*, with their VJPs under CW and one
    dmad_defense_query_logits call per batch of queries under the query-only attacks), or the host operators (torch, and scipy's lfilter
    on the CPU as in the reference).
`--defense None | Diffusion | Diffusion-Spec` belong to the three existing drivers and are refused here with the driver's name; FeCo and
DefenseGAN are not provided.  `run(args, classifier=None, log=print, **attack_overrides)` is importable and returns the accuracy figures."""
import torch

import adaptive_attack_eval as white_box
import black_box_attack_eval as fakebob
import siren_attack_eval as siren

ATTACKS = ['CW', 'FAKEBOB', 'SirenAttack']
DEFENSES = list(white_box.BASELINE_DEFENSES)
_ATTACK_DRIVER = {'CW': 'adaptive_attack_eval.py', 'FAKEBOB': 'black_box_attack_eval.py', 'SirenAttack': 'siren_attack_eval.py'}


def build_parser():
    parser = white_box.build_parser()
    parser.description = __doc__
    # the flags the query-only drivers add to the reference's
    parser.add_argument('--nes_noise', choices=['device', 'torch'], default='device', help='FAKEBOB: the NES probe directions')
    parser.add_argument('--swarm_noise', choices=['device', 'numpy'], default='device', help='SirenAttack: the swarm')
    parser.add_argument('--siren_loss', choices=['reference', 'margin'], default='reference', help='SirenAttack: loss of the swarm')
    parser.add_argument('--seed', type=int, default=0, help='key of the device-side draws of FAKEBOB / SirenAttack')
    parser.add_argument('--defense_backend', choices=['hip', 'host'], default='hip',
                        help="the defense on the engine's kernels, or on the host operators (torch / scipy)")
    return parser


def check_supported(args):
    """NotImplementedError for every attack, defense and option this driver does not run."""
    if args.attack not in ATTACKS:
        raise NotImplementedError('--attack %s: this driver runs CW, FAKEBOB and SirenAttack (Qin-I: imperceptible_attack_eval.py, without a baseline defense; Kenansville, FFT form: '
                                  'kenansville_attack_eval.py, without a baseline defense)' % args.attack)
    if args.defense in ('None', 'Diffusion', 'Diffusion-Spec'):
        raise NotImplementedError('--defense %s: %s runs it under --attack %s, this driver runs the baseline defenses %s'
                                  % (args.defense, _ATTACK_DRIVER[args.attack], args.attack, ', '.join(DEFENSES)))
    if args.defense in white_box._MISSING_DEFENSE:
        raise NotImplementedError('--defense %s needs %s, which this package does not provide (supported here: %s)'
                                  % (args.defense, white_box._MISSING_DEFENSE[args.defense], ', '.join(DEFENSES)))
    if args.defense not in DEFENSES:
        raise NotImplementedError('unknown defense: %s' % args.defense)
    if args.attack == 'CW' and args.max_iter_2 > 0:
        raise NotImplementedError('--max_iter_2 > 0 runs AudioAttack stage 2 (Qin-I): imperceptible_attack_eval.py runs it, this driver does not')


def build_defender(args, engine=None):
    from transforms.frequency_defense import FreqDomainDefense
    from transforms.time_defense import TimeDomainDefense
    kw = dict(backend=args.defense_backend, engine=engine if args.defense_backend == 'hip' else None)
    return TimeDomainDefense(args.defense, **kw) if args.defense in ('AS', 'MS') else FreqDomainDefense(args.defense, **kw)


def run(args, classifier=None, log=print, **attack_overrides):
    """The reference's evaluation loop.  Returns {'total', 'clean_acc', 'denoised_acc', 'robust_acc'} (accuracies in percent)."""
    from acoustic_system import AcousticSystem
    check_supported(args)
    torch.cuda.set_device(args.gpu)
    classifier, wave2spect = white_box.build_front(args, classifier)
    defender = build_defender(args, classifier.__dict__.get('engine'))
    AS_MODEL = AcousticSystem(classifier=classifier, transform=wave2spect, defender=defender, defense_type='wave')
    if args.attack == 'CW':
        if attack_overrides:
            raise TypeError('the CW attacker takes its constants from the flags, not from overrides: %s' % sorted(attack_overrides))
        make_attacker = white_box.attacker_factory(args, AS_MODEL, log)
    else:
        make_attacker = (fakebob if args.attack == 'FAKEBOB' else siren).attacker_factory(args, AS_MODEL, log, **attack_overrides)
    return white_box.evaluate(args, AS_MODEL, classifier, make_attacker, log)


if __name__ == '__main__':
    run(build_parser().parse_args())
