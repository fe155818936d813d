"""SirenAttack driver on the MI355X engine: the SirenAttack branch of the reference's adaptive_attack_eval.py (l.219-227 and its
evaluation loop l.234-370), with the pieces of this package in place of the CUDA ones.

  python siren_attack_eval.py --data_path <SC09 test folder> --attack SirenAttack --defense Diffusion --t 1

It shares its flags, `build_system`, the defense checks and the evaluation loop (`evaluate`) with adaptive_attack_eval.py (the
white-box driver) and accepts only `--attack SirenAttack` (FAKEBOB: black_box_attack_eval.py; Kenansville: its FFT form runs in
kenansville_attack_eval.py, the SSA form is not provided).
`--save_path` writes the clean / purified / adversarial waveforms as 16-bit WAV files, as in the white-box driver.  The attacker is
built with the reference driver's constants: epsilon 0.002, max_epoch 300, max_iter 30, n_particles 25, batches of `--batch_size`
clips, task 'SCR', untargeted.

Additions to the reference's flags:
  * `--swarm_noise {device,numpy}` (default device): where the swarm lives — in four state tensors on the engine, drawn and moved by
    dmad_pso_init / dmad_pso_step / dmad_pso_update_best, or in numpy draws and host loops as in the reference;
  * `--seed`: the key of the device draws;
  * `--siren_loss {reference,margin}` (default reference): the loss the swarm minimises.  The reference's is the cross-entropy of the
    true label, with which the attack never succeeds and the robust accuracy printed is 100 % (robustness_eval/black_box_attack.py
    says why); `margin` is the untargeted margin loss, negative for a misclassified clip.
`run(args, classifier=None, defender=None, log=print, **attack_overrides)` is importable; the overrides replace attacker constants
(tests shrink max_epoch, max_iter and n_particles).  It returns the accuracy figures."""
import torch

import adaptive_attack_eval as white_box

ATTACKER_CONSTANTS = dict(epsilon=0.002, max_epoch=300, max_iter=30, n_particles=25)


def build_parser():
    parser = white_box.build_parser()
    parser.description = __doc__
    parser.add_argument('--swarm_noise', choices=['device', 'numpy'], default='device',
                        help='the swarm: state tensors and Philox draws on the engine, or numpy draws and host loops as in the reference')
    parser.add_argument('--seed', type=int, default=0, help='key of the device-side swarm draws')
    parser.add_argument('--siren_loss', choices=['reference', 'margin'], default='reference',
                        help="loss of the swarm: the reference's cross-entropy of the true label, or the untargeted margin")
    return parser


def check_supported(args):
    """NotImplementedError for anything but SirenAttack, and for a defense / option adaptive_attack_eval.py refuses for every attack."""
    if args.attack != 'SirenAttack':
        raise NotImplementedError('--attack %s: this driver runs SirenAttack only (CW: adaptive_attack_eval.py; FAKEBOB: '
                                  'black_box_attack_eval.py; Qin-I: imperceptible_attack_eval.py; Kenansville, FFT form: kenansville_attack_eval.py)' % args.attack)
    white_box.check_defense(args)


def run(args, classifier=None, defender=None, log=print, **attack_overrides):
    """The reference's evaluation loop.  Returns {'total', 'clean_acc', 'denoised_acc', 'robust_acc'} (accuracies in percent)."""
    check_supported(args)
    torch.cuda.set_device(args.gpu)
    AS_MODEL, classifier = white_box.build_system(args, classifier, defender)
    return white_box.evaluate(args, AS_MODEL, classifier, attacker_factory(args, AS_MODEL, log, **attack_overrides), log)


def attacker_factory(args, AS_MODEL, log=print, **attack_overrides):
    """make_attacker() of evaluate(): the SirenAttack attacker of the driver's flags and constants (shared with baseline_defense_eval.py)."""
    from robustness_eval.black_box_attack import SirenAttack

    def make_attacker():
        k = dict(ATTACKER_CONSTANTS, **attack_overrides)
        Attacker = SirenAttack(model=AS_MODEL, task='SCR', targeted=False, verbose=args.verbose, batch_size=args.batch_size,
                               noise_source=args.swarm_noise, seed=args.seed, loss=args.siren_loss, **k)   # ONE attacker: its draw counter runs on
        log('attack: {} with eps={} & max_epoch={} & iter={} & n_particles={}\n'.format(args.attack, k['epsilon'], k['max_epoch'],
                                                                                      k['max_iter'], k['n_particles']))
        return Attacker
    return make_attacker


if __name__ == '__main__':
    run(build_parser().parse_args())
