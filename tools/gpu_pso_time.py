"""Time and peak memory of one SirenAttack swarm iteration at the driver's settings, the device-side swarm against the numpy path.

  python tools/gpu_pso_time.py [--out FILE]      # one MI355X; prints the table of profiles/r12_pso_device.md

n = 20 clips, 25 particles each (500 query rows per evaluation), epsilon 0.002, EOT 1-1, on AcousticSystem over one exact-vote engine
(max_batch 64, the default of get_engine) with the synthetic calibrated ResNeXt29 (seed 2929) and WaveNet (seed 1234): once without a
defender and once with DiffWave(t = 1) on the DDPM one-call path.  The labels are the runner-up classes, so that the loss is not
identically zero and personal bests do improve (their row copies are part of an iteration).  `device` is SirenAttack(noise_source=
'device'), `numpy` is SirenAttack(noise_source='numpy') of the same commit — the reference's code path, its stand-in here — on the same
system and inputs.  A window is one generate() of ONE epoch of `iters` moves (10 without a defender, 3 with the purifier), i.e.
iters + 1 evaluations, one initialisation and iters moves; the figure is the window's time divided by iters + 1.  One warm-up window
each; then 5 timed windows each, the two paths alternating; host clock around a window that ends in a device synchronise.  Peak memory
is torch.cuda.max_memory_allocated() over the allocation before the window (the engine's workspace is outside torch's allocator and
the same for both)."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, 'diffusion-model-for-audio-defense_amd'), ROOT]

from dmad_hip import engine as E, synth  # noqa: E402

N_CLIPS, PARTICLES, EPSILON, WINDOWS = 20, 25, 0.002, 5
ITERS = {'None': 10, 'DiffWave(t=1)': 3}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('--out', default=None, help='write the figures as JSON')
    args = ap.parse_args()
    from acoustic_system import AcousticSystem
    from audio_models.ConvNets_SpeechCommands.models.resnext import CifarResNeXt
    from diffusion_models.diffwave_ddpm import DiffWave, WaveNetHIP
    from diffusion_models.DiffWave_Unconditional.util import calc_diffusion_hyperparams
    from dmad_hip.transforms import MelSpectrogramDB
    from robustness_eval.black_box_attack import SirenAttack

    eng = E.Engine(max_batch=64, precision=E.EXACT)
    eng.load_wavenet(synth.wavenet_state_dict(1234))
    sd = synth.resnext29_state_dict(2929)
    eng.load_resnext29(sd)
    rx = CifarResNeXt(nlabels=10, in_channels=1)
    rx.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()})
    rx = rx.cuda().eval().bind_engine(eng)
    hp = calc_diffusion_hyperparams(**synth.DIFFUSION_CONFIG)
    x = torch.from_numpy(np.stack([synth.synthetic_clip(i) for i in range(N_CLIPS)])).float().cuda()
    out = {'n': N_CLIPS, 'particles': PARTICLES, 'eot': '1-1', 'engine': 'EXACT, max_batch 64', 'windows': WINDOWS}
    np.random.seed(0)
    for name, iters in ITERS.items():
        den = None if name == 'None' else DiffWave(WaveNetHIP(eng), hp, reverse_timestep=1, seed=17)
        system = AcousticSystem(classifier=rx, transform=MelSpectrogramDB(eng), defender=den, defense_type='wave').eval()
        assert system._engine_chain(True) == (eng, 0 if den is None else 1)           # the one-call query path
        with torch.no_grad():
            y = system(x, False).topk(2, 1).indices[:, 1]
        paths = {k: SirenAttack(system, task='SCR', epsilon=EPSILON, max_epoch=1, max_iter=iters, n_particles=PARTICLES, batch_size=N_CLIPS,
                                verbose=0, noise_source=k, seed=3) for k in ('device', 'numpy')}
        res = {k: {'s_per_iteration': [], 'peak_bytes': []} for k in paths}
        for w in range(WINDOWS + 1):                                                  # window 0 warms every shape up
            for k, att in paths.items():
                torch.cuda.synchronize()
                base = torch.cuda.memory_allocated()
                torch.cuda.reset_peak_memory_stats()
                t0 = time.perf_counter()
                att.generate(x, y, targeted=False)
                torch.cuda.synchronize()
                dt = (time.perf_counter() - t0) / (iters + 1)
                if w:
                    res[k]['s_per_iteration'].append(dt)
                    res[k]['peak_bytes'].append(torch.cuda.max_memory_allocated() - base)
        for k in res:
            res[k]['median_s'] = float(np.median(res[k]['s_per_iteration']))
            res[k]['min_s'], res[k]['max_s'] = min(res[k]['s_per_iteration']), max(res[k]['s_per_iteration'])
            res[k]['peak_MB'] = max(res[k]['peak_bytes']) / 1e6
        res['device_over_numpy_time'] = res['device']['median_s'] / res['numpy']['median_s']
        res['iterations_per_window'] = iters + 1
        out[name] = res
    print('| defense | path | s per iteration: median (min - max of %d windows) | peak memory over baseline |' % WINDOWS)
    print('|---|---|---|---|')
    for name in ITERS:
        for k in ('device', 'numpy'):
            r = out[name][k]
            print('| `%s` | %s | %.4f (%.4f - %.4f) | %.1f MB |' % (name, k, r['median_s'], r['min_s'], r['max_s'], r['peak_MB']))
    for name in ITERS:
        print('%s: device / numpy time %.4f' % (name, out[name]['device_over_numpy_time']))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            json.dump(out, f, indent=1)
    eng.close()


if __name__ == '__main__':
    main()
