"""Kenansville driver on the MI355X engine: the Kenansville branch of the reference's adaptive_attack_eval.py (l.200-208 and its
evaluation loop l.234-370) in the attack's FFT form, with the pieces of this package in place of the CUDA ones.

  python kenansville_attack_eval.py --data_path <SC09 test folder> --attack Kenansville --defense Diffusion --t 1

It shares its flags, `build_system`, the defense checks and the evaluation loop (`evaluate`) with adaptive_attack_eval.py (the
white-box driver) and accepts only `--attack Kenansville` (FAKEBOB: black_box_attack_eval.py; SirenAttack: siren_attack_eval.py).
`--save_path` writes the clean / purified / adversarial waveforms as 16-bit WAV files, as in the white-box driver.  The attacker is
built with the reference driver's constants: max_iter 30, raster_width 100, batches of `--batch_size` clips, untargeted.

The reference's drivers hard-code method='ssa', the float64 SVD of a 15 201 x 800 Hankel matrix on the CPU at batch 1, which this package
does not provide: `--kenan_method ssa` is refused, and the rows this driver prints are those of the attack class's own default, the FFT
form, NOT the paper table's.  Keyword clips at their native length, and clip lengths outside the plan of the engine's FFT pair, are out
of scope.

Additions to the reference's flags:
  * `--kenan_method {fft,ssa}` (default fft): the form of the attack; ssa is refused;
  * `--kenan_backend {device,torch}` (default device): the transforms and the bisection on the engine (dmad_wave_rfft /
    dmad_wave_irfft_threshold / dmad_kenan_update), or torch.fft and the reference's host loop.
`run(args, classifier=None, defender=None, log=print, **attack_overrides)` is importable; the overrides replace attacker constants
(tests shrink max_iter).  It returns the accuracy figures."""
import torch

import adaptive_attack_eval as white_box

ATTACKER_CONSTANTS = dict(max_iter=30, raster_width=100)


def build_parser():
    parser = white_box.build_parser()
    parser.description = __doc__
    parser.add_argument('--kenan_method', choices=['fft', 'ssa'], default='fft',
                        help="form of the attack: fft (the attack class's default), or the reference drivers' ssa, which is not provided")
    parser.add_argument('--kenan_backend', choices=['device', 'torch'], default='device',
                        help="the FFT pair and the bisection on the engine, or torch.fft and the reference's host loop")
    return parser


def check_supported(args):
    """NotImplementedError for anything but Kenansville's FFT form, and for a defense / option adaptive_attack_eval.py refuses for every attack."""
    if args.attack != 'Kenansville':
        raise NotImplementedError('--attack %s: this driver runs Kenansville only (CW: adaptive_attack_eval.py; FAKEBOB: '
                                  'black_box_attack_eval.py; SirenAttack: siren_attack_eval.py; Qin-I: imperceptible_attack_eval.py)' % args.attack)
    if args.kenan_method != 'fft':
        raise NotImplementedError("--kenan_method %s: the SSA form is the reference's CPU SVD (float64, one clip at a time), which this package "
                                  'does not provide; the FFT form (--kenan_method fft) runs' % args.kenan_method)
    white_box.check_defense(args)


def run(args, classifier=None, defender=None, log=print, **attack_overrides):
    """The reference's evaluation loop.  Returns {'total', 'clean_acc', 'denoised_acc', 'robust_acc'} (accuracies in percent)."""
    check_supported(args)
    torch.cuda.set_device(args.gpu)
    AS_MODEL, classifier = white_box.build_system(args, classifier, defender)
    return white_box.evaluate(args, AS_MODEL, classifier, attacker_factory(args, AS_MODEL, log, **attack_overrides), log)


def attacker_factory(args, AS_MODEL, log=print, **attack_overrides):
    """make_attacker() of evaluate(): the Kenansville attacker of the driver's flags and constants."""
    from robustness_eval.black_box_attack import Kenansville

    def make_attacker():
        k = dict(ATTACKER_CONSTANTS, **attack_overrides)
        Attacker = Kenansville(model=AS_MODEL, atk_name=args.kenan_method, targeted=False, verbose=args.verbose, batch_size=args.batch_size,
                               fft_backend=args.kenan_backend, **k)
        log('attack: {} with method={} & iter={} & backend={}\n'.format(args.attack, args.kenan_method, k['max_iter'], args.kenan_backend))
        return Attacker
    return make_attacker


if __name__ == '__main__':
    run(build_parser().parse_args())
