"""Imperceptible-attack driver on the MI355X engine: the Qin-I branch of the reference's adaptive_attack_eval.py (l.193-198, its
evaluation loop l.234-370 and the stage-2 success rate l.348-351, 371-372), with the pieces of this package in place of the CUDA ones.

  python imperceptible_attack_eval.py --data_path <SC09 test folder> --defense Diffusion --t 1 --max_iter_1 10 --max_iter_2 4000

It shares its flags, `build_system`, the defense checks and the evaluation loop (`evaluate`) with adaptive_attack_eval.py (the
white-box driver, which sends Qin-I here) and accepts only `--attack Qin-I`, its default (CW: adaptive_attack_eval.py; FAKEBOB:
black_box_attack_eval.py; SirenAttack: siren_attack_eval.py; Kenansville: its FFT form runs in
kenansville_attack_eval.py, the SSA form is not provided), with `--defense` None, Diffusion or
Diffusion-Spec.  The attacker is the reference driver's: AudioAttack(model, masker=PsychoacousticMasker(), eps, norm, max_iter_1,
max_iter_2, learning_rate_1=eps / 5), untargeted; stage 1 is the CW loop, stage 2 lowers the masking loss of the perturbation
(robustness_eval/white_box_attack.py).  After the reference's accuracy lines it prints the stage-2 success count and rate.

Differences from the reference's flags:
  * `--attack` defaults to Qin-I and `--max_iter_2` to 4000, AudioAttack's own default (the reference's driver defaults to 0, with
    which its Qin-I branch runs stage 1 only); `--max_iter_2 0` is refused: that is adaptive_attack_eval.py's attack;
  * `--eot_attack_size` / `--eot_defense_size` are passed to the attacker (the reference's branch drops them, so that its stage 1
    always runs AudioAttack's default EOT of 15); stage 2 uses no EOT, as in the reference;
  * `--masking_backend {hip,torch}` (default hip): the masking loss, its gradient and the update of stage 2 in one engine call per
    iteration (dmad_masking_step), or the reference's torch operators.
`run(args, classifier=None, defender=None, log=print, **attack_overrides)` is importable; the overrides replace AudioAttack keywords
(tests shorten the alpha periods).  It returns the accuracy figures plus 'imperceptible_success' and 'imperceptible_rate'."""
import adaptive_attack_eval as white_box

_OTHER_DRIVER = dict(white_box._OTHER_DRIVER, CW='adaptive_attack_eval.py')


def build_parser():
    parser = white_box.build_parser()
    parser.description = __doc__
    parser.set_defaults(attack='Qin-I', max_iter_2=4000)
    parser.add_argument('--masking_backend', choices=['hip', 'torch'], default='hip',
                        help="stage 2's masking loss, gradient and update: one engine call per iteration, or the torch operators")
    return parser


def check_supported(args):
    """NotImplementedError for anything but Qin-I with stage 2, and for a defense / option adaptive_attack_eval.py refuses for every attack."""
    if args.attack in _OTHER_DRIVER:
        raise NotImplementedError('--attack %s: this driver runs Qin-I only (%s runs %s)' % (args.attack, _OTHER_DRIVER[args.attack], args.attack))
    if args.attack != 'Qin-I':
        raise NotImplementedError('--attack %s: this driver runs Qin-I only' % args.attack)
    white_box.check_defense(args)
    if args.max_iter_2 <= 0:
        raise NotImplementedError('--max_iter_2 %d: Qin-I without stage 2 is the CW attack of adaptive_attack_eval.py' % args.max_iter_2)


class _CountStage2:
    """the attacker, with the stage-2 successes of every batch summed (evaluate() reads stage 1's only)"""

    def __init__(self, attacker):
        self.attacker, self.success = attacker, 0

    def generate(self, x, y, targeted):
        x_adv, (first, second) = self.attacker.generate(x=x, y=y, targeted=targeted)
        self.success += int(sum(bool(s) for s in second))
        return x_adv, (first, second)


def attacker_factory(args, AS_MODEL, log=print, **attack_overrides):
    """make_attacker() of evaluate(): the Qin-I attacker of the driver's flags (reference l.193-198)."""
    from robustness_eval.white_box_attack import AudioAttack, PsychoacousticMasker

    def make_attacker():
        k = dict(eot_attack_size=args.eot_attack_size, eot_defense_size=args.eot_defense_size, masking_backend=args.masking_backend)
        k.update(attack_overrides)
        attacker = AudioAttack(model=AS_MODEL, masker=PsychoacousticMasker(), eps=args.eps, norm=args.bound_norm, max_iter_1=args.max_iter_1,
                               max_iter_2=args.max_iter_2, learning_rate_1=args.eps / 5, verbose=args.verbose, **k)
        log('attack: {} with {}_eps={} & iter={}+{} & eot={}-{} & masking={}'.format(
            args.attack, args.bound_norm, args.eps, args.max_iter_1, args.max_iter_2, k['eot_attack_size'], k['eot_defense_size'],
            k['masking_backend']))
        make_attacker.last = _CountStage2(attacker)
        return make_attacker.last
    return make_attacker


def run(args, classifier=None, defender=None, log=print, **attack_overrides):
    """The reference's evaluation loop.  Returns evaluate()'s figures plus the stage-2 success count and rate (percent)."""
    import torch
    check_supported(args)
    torch.cuda.set_device(args.gpu)
    AS_MODEL, classifier = white_box.build_system(args, classifier, defender)
    make_attacker = attacker_factory(args, AS_MODEL, log, **attack_overrides)
    out = white_box.evaluate(args, AS_MODEL, classifier, make_attacker, log)
    success = make_attacker.last.success
    rate = success / out['total'] * 100 if out['total'] else 0.0
    log('Imperceptible attack success: {} of {}'.format(success, out['total']))
    log('Imperceptible attack success rate: {:.4f}%'.format(rate))
    return dict(out, imperceptible_success=success, imperceptible_rate=rate)


def main(argv=None, **run_arguments):
    """the command line: `argv` (default sys.argv[1:]) through the parser into run(); keywords go to run() as they are"""
    return run(build_parser().parse_args(argv), **run_arguments)


if __name__ == '__main__':
    main()
