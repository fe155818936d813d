"""Time and memory of the attention-CRNN keyword spotter: the engine (dmad_kws_logits / dmad_kws_vjp) against the torch module's own layers
on the same commit.

  python tools/gpu_kws_time.py [--out FILE]      # one MI355X; prints the tables of profiles/r19_kws.md

KWSModel.use_engine() over one FP32 engine (no WaveNet, no spectrogram classifier) with the trained weights of
tests/golden/kws_vanilla.npz, called on the spectrogram itself: the mel front-end is not on the engine and is not timed.  The torch
side is the same module with no engine in use (MIOpen's GRU under no_grad; torch's own GRU cells under autograd, where MIOpen refuses
an eval-mode backward), in the same process.  Rows are [1,32,81] spectrograms, a 1 s clip.
  * forward, under no_grad, and one CW gradient (forward plus backward of the CW margin loss to the spectrogram, KWSModel.grad_backend
    'hip' against the layers) at B = 1 (the driver's batch), B = 20 and B = 4 020 (one FAKEBOB estimate: 20 clips x 201 probes);
  * time: one warm-up run each, then 7 timed runs each, the two sides alternating.  A run is REPS[B] calls back to back, so that the
    window is milliseconds and not one launch; host clock around a run that ends in a device synchronise, divided by the calls; the
    table gives the median and the min - max spread;
  * memory: torch.cuda.max_memory_allocated over one call (reset before it) less what was resident before it.  The engine has no
    workspace for KWS: its side allocates the results and nothing else."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, 'diffusion-model-for-audio-defense_amd'), ROOT]

from dmad_hip import engine as E  # noqa: E402

T, RUNS = 81, 7
REPS = {1: 50, 20: 50, 4020: 5}


def timed(fn, reps):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / reps


def stats(ts):
    return {'median_ms': 1e3 * float(np.median(ts)), 'min_ms': 1e3 * min(ts), 'max_ms': 1e3 * max(ts)}


def measure(fns, reps):
    """{name: fn} -> ({name: time stats per call}, {name: bytes torch allocated on top of what was resident})"""
    ts = {k: [] for k in fns}
    for k in fns:
        fns[k]()                                                          # warm-up: MIOpen's algorithm search, the allocator's pools
    for _ in range(RUNS):
        for k in fns:
            ts[k].append(timed(fns[k], reps))
    mem = {}
    for k in fns:
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        before = torch.cuda.memory_allocated()
        fns[k]()
        torch.cuda.synchronize()
        mem[k] = int(torch.cuda.max_memory_allocated() - before)
    return {k: stats(v) for k, v in ts.items()}, mem


def cw_loss(logp, y):
    """the CW margin: the best other class over the true one, summed over the batch"""
    true = logp.gather(1, y[:, None])[:, 0]
    other = logp.masked_fill(torch.nn.functional.one_hot(y, logp.shape[1]).bool(), float('-inf')).amax(1)
    return (other - true).clamp_min(0).sum() + 0 * logp.sum()


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('--out', default=None, help='write the figures as JSON')
    args = ap.parse_args()
    from audio_models.RCNN_KWS.model import KWSModel

    with np.load(os.path.join(ROOT, 'tests', 'golden', 'kws_vanilla.npz')) as z:
        sd = {str(k): torch.from_numpy(z['w.' + str(k)]) for k in z['keys']}

    def module():
        m = KWSModel(in_size=32)
        m.load_state_dict(sd)
        return m.cuda().eval()

    eng = E.Engine(max_batch=64, precision=E.FP32, with_wavenet=False, with_classifier=False)
    hip = module().use_engine(eng)
    hip.grad_backend = 'hip'
    systems = {'hip': hip, 'torch': module()}
    gen = torch.Generator().manual_seed(81)
    base = (torch.randn(20, 1, 32, T, generator=gen) * 15 - 30).cuda()
    out = {'runs': RUNS, 'reps': REPS, 'T': T, 'engine': 'FP32, no WaveNet, no spectrogram classifier', 'forward': {}, 'gradient': {}}
    for B in REPS:
        xb = (base[:1] if B == 1 else base.repeat(B // 20, 1, 1, 1)).contiguous()
        with torch.no_grad():
            y = systems['torch'](xb).argmin(1)              # a target the clip is not at: the margin is active

        def forward(system):
            with torch.no_grad():
                return system(xb)

        def grad(system):
            xi = xb.clone().requires_grad_(True)
            cw_loss(system(xi), y).backward()
            system.zero_grad(set_to_none=True)
            return xi.grad

        t, m = measure({k: (lambda s=s: forward(s)) for k, s in systems.items()}, REPS[B])
        out['forward'][str(B)] = {'time': t, 'bytes': m}
        t, m = measure({k: (lambda s=s: grad(s)) for k, s in systems.items()}, REPS[B])
        out['gradient'][str(B)] = {'time': t, 'bytes': m}
        gh, gt = grad(systems['hip']), grad(systems['torch'])
        out['gradient'][str(B)]['hip_vs_torch'] = float((gh - gt).abs().max() / gt.abs().max())
    for what in ('forward', 'gradient'):
        print('\n| %s rows | hip median ms (min - max) | torch median ms (min - max) | torch / hip | hip MB allocated | torch MB allocated |\n'
              '|---|---|---|---|---|---|' % what)
        for B, v in out[what].items():
            h, t = v['time']['hip'], v['time']['torch']
            print('| %s | %.3f (%.3f - %.3f) | %.3f (%.3f - %.3f) | %.2f | %.3f | %.3f |'
                  % (B, h['median_ms'], h['min_ms'], h['max_ms'], t['median_ms'], t['min_ms'], t['max_ms'], t['median_ms'] / h['median_ms'],
                     v['bytes']['hip'] / 1e6, v['bytes']['torch'] / 1e6))
    print('\ngradient, hip against torch, of its maximum: %s' % {B: '%.2e' % v['hip_vs_torch'] for B, v in out['gradient'].items()})
    print('engine MB (dmad_device_bytes): %.1f' % (eng.device_bytes() / 1e6))
    if args.out:
        with open(args.out, 'w') as f:
            json.dump(out, f, indent=1)
    eng.close()


if __name__ == '__main__':
    main()
