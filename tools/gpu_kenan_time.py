#!/usr/bin/env python3
"""Times the whole-clip FFT pair of the engine against torch.fft (rocFFT) and one iteration of the Kenansville FFT attack on both
backends (profiles/r25_kenansville.md).  FP32 engine, L = 16000, medians of 7 runs after 3 warm-up runs, HIP events on the current stream.

  python tools/gpu_kenan_time.py [--out FILE]

Rows: wave_rfft / wave_irfft_threshold at B = 1, 20 and 4020 against torch.fft.rfft / the masked assignment + torch.fft.irfft; one attack
iteration (thresholded inverse, the system's scores, arg-max, bisection update) at B = 20 against the synthetic VGG19_bn behind the mel
front-end, without a purifier and behind DiffWave(t = 1) on the DDPM one-call path, on both backends, with the query alone beside them;
torch allocations over that iteration."""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'diffusion-model-for-audio-defense_amd'))
L, RUNS, WARM = 16000, 7, 3


def median_ms(fn):
    for _ in range(WARM):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(RUNS):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return float(np.median(ms))


def allocations(fn):
    fn()
    torch.cuda.synchronize()
    before = torch.cuda.memory_stats()['allocation.all.allocated']
    fn()
    torch.cuda.synchronize()
    return int(torch.cuda.memory_stats()['allocation.all.allocated'] - before)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('--out', default=None, help='also write the JSON result here')
    args = ap.parse_args()
    from acoustic_system import AcousticSystem
    from audio_models.ConvNets_SpeechCommands.models.vgg import vgg19_bn
    from diffusion_models.diffwave_ddpm import DiffWave, WaveNetHIP
    from diffusion_models.DiffWave_Unconditional.util import calc_diffusion_hyperparams
    from dmad_hip import engine as E
    from dmad_hip import synth
    from dmad_hip.transforms import MelSpectrogramDB
    from robustness_eval import _KenanFFT as K

    res = {'L': L, 'runs': RUNS, 'device': torch.cuda.get_device_name(0), 'fft': [], 'iteration': []}
    e = E.Engine(max_batch=32, precision=E.FP32)
    e.load_wavenet(synth.wavenet_state_dict(1234))
    sd = synth.vgg19_bn_state_dict(4321)
    e.load_vgg19_bn(sd)
    gen = torch.Generator().manual_seed(0)
    for B in (1, 20, 4020):
        x = (0.3 * torch.randn(B, L, generator=gen)).cuda()
        spec, maxmag = e.wave_rfft(x)
        f = (0.01 * maxmag).contiguous()
        out, kept = e.wave_irfft_threshold(spec, f)
        X = torch.fft.rfft(x, dim=1)

        def torch_inverse():
            Y = X.clone()
            Y[Y.abs() < f.unsqueeze(1)] = 0
            return torch.fft.irfft(Y, dim=1)

        def torch_forward():
            return torch.fft.fft(x, dim=1).abs().max(dim=1)[0], torch.fft.rfft(x, dim=1)
        res['fft'].append({'B': B,
                           'wave_rfft_ms': median_ms(lambda: e.wave_rfft(x)),
                           'torch_rfft_ms': median_ms(lambda: torch.fft.rfft(x, dim=1)),
                           'torch_fft_absmax_and_rfft_ms': median_ms(torch_forward),
                           'wave_irfft_threshold_ms': median_ms(lambda: e.wave_irfft_threshold(spec, f, out, kept)),
                           'torch_mask_irfft_ms': median_ms(torch_inverse)})
        print(json.dumps(res['fft'][-1]), flush=True)

    net = vgg19_bn(num_classes=10, in_channels=1)
    net.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()})
    net = net.cuda().eval().bind_engine(e)
    hp = calc_diffusion_hyperparams(**synth.DIFFUSION_CONFIG)
    B = 20
    x = torch.from_numpy(np.stack([synth.synthetic_clip(i) for i in range(B)])).float().cuda()
    for name in ('None', 'DiffWave(t=1)'):
        den = None if name == 'None' else DiffWave(WaveNetHIP(e), hp, reverse_timestep=1, seed=17)
        system = AcousticSystem(classifier=net, transform=MelSpectrogramDB(e), defender=den, defense_type='wave').eval()
        assert system._engine_chain(True) == (e, 0 if den is None else 1)          # the one-call query path
        with torch.no_grad():
            y = system(x, False).argmax(1)
        scores = lambda q, system=system: system.query(q, 1, per_call=1)[0][0]      # noqa: E731
        spec, upper = e.wave_rfft(x[:, 0])
        state = dict(lower=torch.zeros_like(upper), upper=upper.clone(), factor=upper / 2, best=x[:, 0].clone(),
                     succ=torch.zeros(B, device='cuda', dtype=torch.int32), perturbed=None, kept=None)

        def device_iteration():
            s = state
            s['perturbed'], s['kept'] = e.wave_irfft_threshold(spec, s['factor'], s['perturbed'], s['kept'])
            pred = scores(s['perturbed'].view(B, 1, L)).max(1)[1].long()
            e.kenan_update(pred, y, False, s['perturbed'], s['best'], s['lower'], s['upper'], s['factor'], s['succ'])

        def query_only():
            scores(x)

        def torch_iteration():
            with torch.no_grad():
                K.atk_bst_fft(x, y, False, scores, 1)                  # one iteration, its own set-up (fft, abs, max) included
        res['iteration'].append({'defender': name, 'B': B, 'device_ms': median_ms(device_iteration), 'torch_ms': median_ms(torch_iteration),
                                 'query_alone_ms': median_ms(query_only), 'device_allocations': allocations(device_iteration),
                                 'torch_allocations': allocations(torch_iteration), 'query_allocations': allocations(query_only)})
        print(json.dumps(res['iteration'][-1]), flush=True)
    e.close()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as fh:
            json.dump(res, fh, indent=1)


if __name__ == '__main__':
    main()
