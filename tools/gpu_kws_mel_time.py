"""Time and memory of the keyword spotter behind its mel front-end: the engine's fused route (dmad_kws_wave_logits / dmad_kws_wave_vjp,
read frames only) against the engine's two-call route (dmad_kws_mel_db + dmad_kws_logits, dmad_kws_vjp + dmad_kws_mel_db_vjp, all
frames) and against the torch branch (dmad_hip.autograd.kws_mel_db + the module's own layers) on the same commit.

  python tools/gpu_kws_mel_time.py [--out FILE]      # one MI355X; prints the tables of profiles/r20_kws_mel.md

One FP32 engine (no WaveNet, no spectrogram classifier) with the trained weights of tests/golden/kws_vanilla.npz; clips of L = 16000
samples (T = 81 frames, 25 of them read), all three sides in the same process:
  * the front-end alone (waveform -> dB spectrogram, all frames: engine kws_mel_db against autograd.kws_mel_db), waveform -> logp under
    no_grad, and one CW gradient (forward plus backward of the CW margin loss to the waveform) at B = 1 (the driver's batch), B = 20 and
    B = 4 020 (one FAKEBOB estimate: 20 clips x 201 probes);
  * time: one warm-up run each, then 7 timed runs each, the sides alternating.  A run is REPS[B] calls back to back; host clock around a
    run that ends in a device synchronise, divided by the calls; the table gives the median and the min - max spread;
  * memory: torch.cuda.max_memory_allocated over one gradient (reset before it) less what was resident before it."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, 'diffusion-model-for-audio-defense_amd'), ROOT]

from dmad_hip import autograd as ag  # noqa: E402
from dmad_hip import engine as E  # noqa: E402

L, RUNS = 16000, 7
REPS = {1: 50, 20: 20, 4020: 3}
SIDES = ('fused', 'two_call', 'torch')


def timed(fn, reps):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / reps


def stats(ts):
    return {'median_ms': 1e3 * float(np.median(ts)), 'min_ms': 1e3 * min(ts), 'max_ms': 1e3 * max(ts)}


def measure(fns, reps, memory=False):
    """{name: fn} -> ({name: time stats per call}, {name: bytes torch allocated on top of what was resident})"""
    ts = {k: [] for k in fns}
    for k in fns:
        fns[k]()                                                          # warm-up: plans, MIOpen's search, the allocator's pools
    for _ in range(RUNS):
        for k in fns:
            ts[k].append(timed(fns[k], reps))
    mem = {}
    for k in fns if memory else ():
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        before = torch.cuda.memory_allocated()
        fns[k]()
        torch.cuda.synchronize()
        mem[k] = int(torch.cuda.max_memory_allocated() - before)
    return {k: stats(v) for k, v in ts.items()}, mem


def cw_grad(logp, y):
    """the gradient of the CW margin (the best other class over the true one, summed over the batch) at logp"""
    lp = logp.detach().requires_grad_(True)
    true = lp.gather(1, y[:, None])[:, 0]
    other = lp.masked_fill(torch.nn.functional.one_hot(y, lp.shape[1]).bool(), float('-inf')).amax(1)
    ((other - true).clamp_min(0).sum() + 0 * lp.sum()).backward()
    return lp.grad


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('--out', default=None, help='write the figures as JSON')
    args = ap.parse_args()
    from audio_models.RCNN_KWS.model import KWSModel

    with np.load(os.path.join(ROOT, 'tests', 'golden', 'kws_vanilla.npz')) as z:
        sd = {str(k): torch.from_numpy(z['w.' + str(k)]) for k in z['keys']}
    eng = E.Engine(max_batch=64, precision=E.FP32, with_wavenet=False, with_classifier=False)
    eng.load_kws(sd)
    net = KWSModel(in_size=32)
    net.load_state_dict(sd)
    net = net.cuda().eval()
    gen = torch.Generator().manual_seed(16000)
    base = (torch.randn(20, 1, L, generator=gen) * 0.1).cuda()
    out = {'runs': RUNS, 'reps': REPS, 'L': L, 'engine': 'FP32, no WaveNet, no spectrogram classifier', 'front_end': {}, 'forward': {}, 'gradient': {}}
    for B in REPS:
        xb = (base[:1] if B == 1 else base.repeat(B // 20, 1, 1)).contiguous()
        with torch.no_grad():
            y = eng.kws_wave_logits(xb).argmin(1)           # a target the clip is not at: the margin is active

        def torch_forward(x):
            return net(ag.kws_mel_db(x))

        def torch_grad():
            xi = xb.clone().requires_grad_(True)
            lp = torch_forward(xi)
            lp.backward(cw_grad(lp, y))
            net.zero_grad(set_to_none=True)
            return xi.grad[:, 0]

        def fused_grad():
            return eng.kws_wave_vjp(xb, cw_grad(eng.kws_wave_logits(xb), y))

        def two_call_grad():
            db = eng.kws_mel_db(xb)
            return eng.kws_mel_db_vjp(xb, eng.kws_vjp(db, cw_grad(eng.kws_logits(db), y)))

        with torch.no_grad():
            t, _ = measure({'engine': lambda: eng.kws_mel_db(xb), 'torch': lambda: ag.kws_mel_db(xb)}, REPS[B])
            out['front_end'][str(B)] = {'time': t}
            t, _ = measure({'fused': lambda: eng.kws_wave_logits(xb), 'two_call': lambda: eng.kws_logits(eng.kws_mel_db(xb)),
                            'torch': lambda: torch_forward(xb)}, REPS[B])
            out['forward'][str(B)] = {'time': t}
        t, m = measure({'fused': fused_grad, 'two_call': two_call_grad, 'torch': torch_grad}, REPS[B], memory=True)
        gt = torch_grad()
        out['gradient'][str(B)] = {'time': t, 'bytes': m, 'fused_equals_two_call': bool(torch.equal(fused_grad(), two_call_grad())),
                                   'fused_vs_torch': float((fused_grad() - gt).abs().max() / gt.abs().max())}
    print('\n| front-end rows | engine median ms (min - max) | torch median ms (min - max) | torch / engine |\n|---|---|---|---|')
    for B, v in out['front_end'].items():
        h, t = v['time']['engine'], v['time']['torch']
        print('| %s | %.3f (%.3f - %.3f) | %.3f (%.3f - %.3f) | %.2f |' % (B, h['median_ms'], h['min_ms'], h['max_ms'], t['median_ms'], t['min_ms'],
                                                                         t['max_ms'], t['median_ms'] / h['median_ms']))
    for what in ('forward', 'gradient'):
        print('\n| %s rows | fused median ms (min - max) | two-call median ms (min - max) | torch median ms (min - max) | two-call / fused | torch / fused |'
              '%s\n|---|---|---|---|---|---|%s' % (what, ' fused MB | two-call MB | torch MB |' if what == 'gradient' else '', '---|---|---|' if what == 'gradient' else ''))
        for B, v in out[what].items():
            f, c, t = (v['time'][k] for k in SIDES)
            row = '| %s | %.3f (%.3f - %.3f) | %.3f (%.3f - %.3f) | %.3f (%.3f - %.3f) | %.2f | %.2f |' % (
                B, f['median_ms'], f['min_ms'], f['max_ms'], c['median_ms'], c['min_ms'], c['max_ms'], t['median_ms'], t['min_ms'], t['max_ms'],
                c['median_ms'] / f['median_ms'], t['median_ms'] / f['median_ms'])
            if what == 'gradient':
                row += ' %.3f | %.3f | %.3f |' % tuple(v['bytes'][k] / 1e6 for k in SIDES)
            print(row)
    print('\ngradient: fused equals two-call bit for bit: %s; fused against torch, of its maximum: %s'
          % ({B: v['fused_equals_two_call'] for B, v in out['gradient'].items()}, {B: '%.2e' % v['fused_vs_torch'] for B, v in out['gradient'].items()}))
    print('engine MB (dmad_device_bytes): %.1f' % (eng.device_bytes() / 1e6))
    if args.out:
        with open(args.out, 'w') as f:
            json.dump(out, f, indent=1)
    eng.close()


if __name__ == '__main__':
    main()
