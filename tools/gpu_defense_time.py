"""Time of the five baseline waveform defenses on the engine against the 'host' backend of the same commit.

  python tools/gpu_defense_time.py [--out FILE]      # one MI355X; prints the tables of profiles/r13_wave_defenses.md

For each of AS, MS, DS, LPF, BPF, on AcousticSystem over one FP32 engine (max_batch 64) with the synthetic calibrated ResNeXt29
(seed 2929), B = 20 synthetic clips:
  * query: 4 020 rows (one FAKEBOB estimate at the driver's settings: 20 clips x 201 probes) as AcousticSystem.query(x, repeats = 201),
    the one-call path of backend 'hip' (dmad_defense_query_logits) against the forward() loop of backend 'host';
  * gradient: one CW gradient, forward plus backward of the cross-entropy through defense -> mel dB -> ResNeXt29, on both backends (the
    last two stages are the engine's VJPs in both; only the defense differs);
  * op: the defense's kernel(s) alone on 4 020 rows, forward and VJP, with the effective GB/s (4 B read + 4 B written per sample of the
    op's input and output rows) against the 8 TB/s of HBM.
One warm-up run each, then 5 timed runs each, the two backends alternating; host clock around a run that ends in a device synchronise;
the table gives the median and the min - max spread."""
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

N_CLIPS, REPEATS, RUNS = 20, 201, 5
HBM_GBS = 8000.0


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0


def stats(ts):
    return {'median_ms': 1e3 * float(np.median(ts)), 'min_ms': 1e3 * min(ts), 'max_ms': 1e3 * max(ts)}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('--out', default=None, help='write the figures as JSON')
    args = ap.parse_args()
    from acoustic_system import AcousticSystem
    from audio_models.ConvNets_SpeechCommands.models.resnext import CifarResNeXt
    from dmad_hip.transforms import MelSpectrogramDB
    from transforms import _wave_design as wd
    from transforms.frequency_defense import FreqDomainDefense
    from transforms.time_defense import TimeDomainDefense

    eng = E.Engine(max_batch=64, precision=E.FP32, with_wavenet=False)
    sd = synth.resnext29_state_dict(2929)
    eng.load_resnext29(sd)
    rx = CifarResNeXt(nlabels=10, in_channels=1)
    rx.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()})
    rx = rx.cuda().eval().bind_engine(eng)
    rx.grad_backend = 'hip'
    x = torch.from_numpy(np.stack([synth.synthetic_clip(i) for i in range(N_CLIPS)])).float().cuda()
    big = x[:, 0].repeat(REPEATS, 1).contiguous()
    gbig = torch.randn_like(big)
    (dk, dw, do, _), (uk, uw, uo, _) = wd.sinc_resample_kernel(16000, 8000), wd.sinc_resample_kernel(8000, 16000)
    lb, la = wd.butter_lowpass(16000, 4000, 8000, 3, 40)[:2]
    bb, ba = wd.butter_bandpass(16000, (300, 4000), (50, 8000), 3, 40)[:2]
    half = big[:, :8000].contiguous()
    ops = {        # name -> (forward, VJP, floats moved per row)
        'AS': (lambda: eng.wave_smooth(big, 0, 3), lambda: eng.wave_smooth_vjp(big, gbig, 0, 3), 32000),
        'MS': (lambda: eng.wave_smooth(big, 1, 3), lambda: eng.wave_smooth_vjp(big, gbig, 1, 3), 32000),
        'DS down': (lambda: eng.wave_resample(big, dk, do, dw, 8000), lambda: eng.wave_resample_vjp(gbig[:, :8000], 16000, dk, do, dw), 24000),
        'DS up': (lambda: eng.wave_resample(half, uk, uo, uw, 16000), lambda: eng.wave_resample_vjp(gbig, 8000, uk, uo, uw), 24000),
        'LPF': (lambda: eng.wave_iir(big, lb, la, -1, 1), lambda: eng.wave_iir_vjp(big, gbig, lb, la, -1, 1), 32000),
        'BPF': (lambda: eng.wave_iir(big, bb, ba, -1, 1), lambda: eng.wave_iir_vjp(big, gbig, bb, ba, -1, 1), 32000),
    }
    out = {'clips': N_CLIPS, 'rows': N_CLIPS * REPEATS, 'runs': RUNS, 'engine': 'FP32, max_batch 64', 'query': {}, 'gradient': {}, 'op': {}}
    for name, (fwd, vjp, floats) in ops.items():
        for what, fn in (('forward', fwd), ('vjp', vjp)):
            fn()
            s = stats([timed(fn) for _ in range(RUNS)])
            moved = floats * 4 * big.shape[0] * (1.0 if what == 'forward' or name in ('AS', 'DS down', 'DS up') else 1.5)   # MS / IIR VJP read x too
            s['gbs'] = moved / (s['median_ms'] * 1e-3) / 1e9
            s['hbm_share'] = s['gbs'] / HBM_GBS
            out['op']['%s %s' % (name, what)] = s
    y = None
    for kind in ('AS', 'MS', 'DS', 'LPF', 'BPF'):
        cls = TimeDomainDefense if kind in ('AS', 'MS') else FreqDomainDefense
        systems = {b: AcousticSystem(classifier=rx, transform=MelSpectrogramDB(eng, grad_backend='hip'),
                                     defender=cls(kind, backend=b, engine=eng if b == 'hip' else None)).eval() for b in ('hip', 'host')}
        assert systems['hip']._engine_chain(True) == (eng, 4) and systems['host']._engine_chain(True) == (None, 0)
        if y is None:
            with torch.no_grad():
                y = systems['hip'](x, False).argmax(1)

        def grad(system):
            xi = x.clone().requires_grad_(True)
            torch.nn.functional.cross_entropy(system(xi), y).backward()
            return xi.grad
        q = {b: [] for b in systems}
        g = {b: [] for b in systems}
        for b, s in systems.items():
            s.query(x, REPEATS, per_call=REPEATS)
            grad(s)
        for _ in range(RUNS):
            for b, s in systems.items():
                q[b].append(timed(lambda: s.query(x, REPEATS, per_call=REPEATS)))
                g[b].append(timed(lambda: grad(s)))
        out['query'][kind] = {b: stats(q[b]) for b in systems}
        out['gradient'][kind] = {b: stats(g[b]) for b in systems}
    print('| op (4 020 rows) | median ms | min - max ms | GB/s | of 8 TB/s |\n|---|---|---|---|---|')
    for k, s in out['op'].items():
        print('| %s | %.3f | %.3f - %.3f | %.0f | %.1f %% |' % (k, s['median_ms'], s['min_ms'], s['max_ms'], s['gbs'], 100 * s['hbm_share']))
    for what in ('query', 'gradient'):
        print('\n| %s | hip median ms (min - max) | host median ms (min - max) | host / hip |\n|---|---|---|---|' % what)
        for k, v in out[what].items():
            h, c = v['hip'], v['host']
            print('| %s | %.2f (%.2f - %.2f) | %.2f (%.2f - %.2f) | %.2f |' % (k, h['median_ms'], h['min_ms'], h['max_ms'], c['median_ms'], c['min_ms'],
                                                                             c['max_ms'], c['median_ms'] / h['median_ms']))
    if args.out:
        with open(args.out, 'w') as f:
            json.dump(out, f, indent=1)
    eng.close()


if __name__ == '__main__':
    main()
