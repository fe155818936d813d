"""Black-box (query-only) attack driver on the MI355X engine: the FAKEBOB branch of the reference's adaptive_attack_eval.py
(l.209-218 and its evaluation loop l.234-370), with the pieces of this package in place of the CUDA ones.

  python black_box_attack_eval.py --data_path <SC09 test folder> --attack FAKEBOB --defense Diffusion --t 1

It shares its flags, `build_system`, the defense checks and the evaluation loop (`evaluate`) with adaptive_attack_eval.py (the
white-box driver, which sends FAKEBOB here) and accepts only `--attack FAKEBOB` (SirenAttack: siren_attack_eval.py; Kenansville: its
FFT form runs in kenansville_attack_eval.py, the SSA form is not provided).
`--save_path` writes the clean / purified / adversarial waveforms as 16-bit WAV files, as in the white-box driver (refused with
`--defense Diffusion-Spec`, whose spectrogram images need a plotting library).  The attacker is built with the
reference driver's constants: epsilon 0.002, confidence 0.5, max_iter 200, samples_per_draw 200 in one draw batch, max_lr 5e-4,
min_lr 1e-4, batches of `--batch_size` clips, task 'SCR', untargeted.

Additions to the reference's flags:
  * `--nes_noise {device,torch}` (default device): where the NES probe directions come from — Philox draws made and consumed on the
    engine (dmad_nes_probes / dmad_nes_grad), or torch.randn tensors as in the reference;
  * `--seed`: the key of the device draws.
`run(args, classifier=None, defender=None, log=print, **attack_overrides)` is importable; the overrides replace attacker constants
(tests shrink max_iter and samples_per_draw).  It returns the accuracy figures."""
import torch

import adaptive_attack_eval as white_box

ATTACKER_CONSTANTS = dict(epsilon=0.002, confidence=0.5, max_iter=200, samples_per_draw=200, max_lr=5e-4, min_lr=1e-4)


def build_parser():
    parser = white_box.build_parser()
    parser.description = __doc__
    parser.add_argument('--nes_noise', choices=['device', 'torch'], default='device',
                        help='NES probe directions: Philox draws on the engine, or torch.randn tensors as in the reference')
    parser.add_argument('--seed', type=int, default=0, help='key of the device-side NES draws')
    return parser


def check_supported(args):
    """NotImplementedError for anything but FAKEBOB, and for a defense / option adaptive_attack_eval.py refuses for every attack."""
    if args.attack != 'FAKEBOB':
        raise NotImplementedError('--attack %s: this driver runs FAKEBOB only (CW: adaptive_attack_eval.py; SirenAttack: '
                                  'siren_attack_eval.py; Qin-I: imperceptible_attack_eval.py; Kenansville, FFT form: kenansville_attack_eval.py)' % args.attack)
    white_box.check_defense(args)


def run(args, classifier=None, defender=None, log=print, **attack_overrides):
    """The reference's evaluation loop.  Returns {'total', 'clean_acc', 'denoised_acc', 'robust_acc'} (accuracies in percent)."""
    check_supported(args)
    torch.cuda.set_device(args.gpu)
    AS_MODEL, classifier = white_box.build_system(args, classifier, defender)
    return white_box.evaluate(args, AS_MODEL, classifier, attacker_factory(args, AS_MODEL, log, **attack_overrides), log)


def attacker_factory(args, AS_MODEL, log=print, **attack_overrides):
    """make_attacker() of evaluate(): the FAKEBOB attacker of the driver's flags and constants (shared with baseline_defense_eval.py)."""
    from robustness_eval.black_box_attack import FAKEBOB

    def make_attacker():
        k = dict(ATTACKER_CONSTANTS, **attack_overrides)
        k.setdefault('samples_per_draw_batch_size', k['samples_per_draw'])
        Attacker = FAKEBOB(model=AS_MODEL, task='SCR', targeted=False, verbose=args.verbose, batch_size=args.batch_size,
                           noise_source=args.nes_noise, seed=args.seed, **k)      # ONE attacker for all batches: its draw counter runs on
        log('attack: {} with eps={} & confidence={} & iter={} & samples_per_draw={}\n'.format(args.attack, k['epsilon'], k['confidence'],
                                                                                            k['max_iter'], k['samples_per_draw']))
        return Attacker
    return make_attacker


if __name__ == '__main__':
    run(build_parser().parse_args())
