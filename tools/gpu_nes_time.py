"""Time and peak memory of one NES estimate at the black-box driver's settings, device-side probe directions against the tensor path.

  python tools/gpu_nes_time.py [--baseline FILE] [--out FILE]      # one MI355X; prints the table of profiles/r11_nes_device.md

n = 20 clips, P = 200 probes in one draw batch (4 020 queries with the unperturbed clips), sigma = 1e-3, EOT 1-1, on AcousticSystem over one
exact-vote engine (max_batch 64, the default of get_engine) with the synthetic calibrated ResNeXt29 (seed 2929) and WaveNet (seed 1234):
once without a defender and once with DiffWave(t = 1) on the DDPM one-call path.  `device` is NES(noise_source='device') with its default
probe_rows; `tensor` is NES(noise_source='torch'), or the NES class of --baseline FILE (an earlier revision of robustness_eval/_NES.py,
to time that very code).  One warm-up estimate each; then 5 timed windows each, the two paths alternating, a window being as many estimates
as take about 2 s or more (5 without a defender, 1 with the purifier); host clock around a window that ends in a device synchronise.  Peak
memory is torch.cuda.max_memory_allocated() over the allocation before the window (the engine's workspace is outside torch's allocator and
the same for both)."""
import argparse
import importlib.util
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, 'diffusion-model-for-audio-defense_amd'), ROOT]

from dmad_hip import engine as E, synth  # noqa: E402

N_CLIPS, PROBES, SIGMA, WINDOWS = 20, 200, 1e-3, 5
PER_WINDOW = {'None': 5, 'DiffWave(t=1)': 1}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('--baseline', default=None, help='a Python file with another NES class to time as the tensor path')
    ap.add_argument('--out', default=None, help='write the figures as JSON')
    args = ap.parse_args()
    from acoustic_system import AcousticSystem
    from audio_models.ConvNets_SpeechCommands.models.resnext import CifarResNeXt
    from diffusion_models.diffwave_ddpm import DiffWave, WaveNetHIP
    from diffusion_models.DiffWave_Unconditional.util import calc_diffusion_hyperparams
    from dmad_hip.transforms import MelSpectrogramDB
    from robustness_eval._EOT import EOT
    from robustness_eval._NES import NES
    from robustness_eval._utils import resolve_loss
    tensor_nes = lambda eot: NES(PROBES, PROBES, SIGMA, eot, noise_source='torch')
    if args.baseline:
        spec = importlib.util.spec_from_file_location('baseline_nes', args.baseline)
        mod = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(mod)
        tensor_nes = lambda eot: mod.NES(PROBES, PROBES, SIGMA, eot)

    eng = E.Engine(max_batch=64, precision=E.EXACT)
    eng.load_wavenet(synth.wavenet_state_dict(1234))
    sd = synth.resnext29_state_dict(2929)
    eng.load_resnext29(sd)
    rx = CifarResNeXt(nlabels=10, in_channels=1)
    rx.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()})
    rx = rx.cuda().eval().bind_engine(eng)
    hp = calc_diffusion_hyperparams(**synth.DIFFUSION_CONFIG)
    x = torch.from_numpy(np.stack([synth.synthetic_clip(i) for i in range(N_CLIPS)])).float().cuda()
    loss_fn, _ = resolve_loss('Margin', False, 0.5, 'SCR', None, False)
    out = {'n': N_CLIPS, 'P': PROBES, 'eot': '1-1', 'engine': 'EXACT, max_batch 64', 'windows': WINDOWS, 'tensor_path': args.baseline or "NES('torch')"}
    for name, per_window in PER_WINDOW.items():
        den = None if name == 'None' else DiffWave(WaveNetHIP(eng), hp, reverse_timestep=1, seed=17)
        system = AcousticSystem(classifier=rx, transform=MelSpectrogramDB(eng), defender=den, defense_type='wave').eval()
        assert system._engine_chain(True) == (eng, 0 if den is None else 1)           # the one-call query path
        with torch.no_grad():
            y = system(x, False).argmax(1)
        eot = EOT(system, loss_fn, 1, 1, False)
        paths = {'device': NES(PROBES, PROBES, SIGMA, eot, noise_source='device', seed=3), 'tensor': tensor_nes(eot)}
        res = {k: {'s_per_estimate': [], 'peak_bytes': []} for k in paths}
        for w in range(WINDOWS + 1):                                                  # window 0 warms every shape up
            for k, nes in paths.items():
                torch.cuda.synchronize()
                base = torch.cuda.memory_allocated()
                torch.cuda.reset_peak_memory_stats()
                t0 = time.perf_counter()
                with torch.no_grad():
                    for _ in range(per_window if w else 1):
                        nes(x, y)
                torch.cuda.synchronize()
                dt = (time.perf_counter() - t0) / (per_window if w else 1)
                if w:
                    res[k]['s_per_estimate'].append(dt)
                    res[k]['peak_bytes'].append(torch.cuda.max_memory_allocated() - base)
        for k in res:
            res[k]['median_s'] = float(np.median(res[k]['s_per_estimate']))
            res[k]['min_s'], res[k]['max_s'] = min(res[k]['s_per_estimate']), max(res[k]['s_per_estimate'])
            res[k]['peak_MB'] = max(res[k]['peak_bytes']) / 1e6
        res['device_over_tensor_time'] = res['device']['median_s'] / res['tensor']['median_s']
        res['estimates_per_window'] = per_window
        out[name] = res
    print('| defense | path | s per estimate: median (min - max of %d windows) | peak memory over baseline |' % WINDOWS)
    print('|---|---|---|---|')
    for name in PER_WINDOW:
        for k in ('device', 'tensor'):
            r = out[name][k]
            print('| `%s` | %s | %.4f (%.4f - %.4f) | %.1f MB |' % (name, k, r['median_s'], r['min_s'], r['max_s'], r['peak_MB']))
    for name in PER_WINDOW:
        print('%s: device / tensor time %.4f' % (name, out[name]['device_over_tensor_time']))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            json.dump(out, f, indent=1)
    eng.close()


if __name__ == '__main__':
    main()
