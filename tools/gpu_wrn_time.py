"""Time and memory of WideResNet-28-10 on the engine: the forward, and one CW gradient through the engine's VJP against the torch branch.

  python tools/gpu_wrn_time.py [--out FILE]      # one MI355X; prints the tables of profiles/r18_wrn.md

AcousticSystem(WideResNet, MelSpectrogramDB, None) over one FP32 engine (max_batch 64, the drivers' default) with the synthetic calibrated
WideResNet-28-10 (seed 2810).
  * forward: dmad_classify on B = 1, 20 and 64 spectrograms against the module's own layers under no_grad (MIOpen), 7 timed runs each
    after a warm-up, the two alternating; host clock around a run that ends in a device synchronise; median and min - max;
  * one CW gradient = forward plus backward of the cross-entropy through mel dB -> WideResNet, at B = 20 (the driver's batch) and B = 300
    (EOT 15 x 20), for grad_backend 'hip' (dmad_wrn_vjp) and 'torch' (the module's own layers and a torch activation tape); the mel
    front-end is the engine's VJP in both;
  * memory: torch.cuda.max_memory_allocated over one gradient (reset before it) next to dmad_device_bytes after it."""
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

BATCHES, FWD_BATCHES, RUNS = (20, 300), (1, 20, 64), 7


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0


def stats(ts):
    return {'median_ms': 1e3 * float(np.median(ts)), 'min_ms': 1e3 * min(ts), 'max_ms': 1e3 * max(ts)}


def row(v):
    return '%.2f (%.2f - %.2f)' % (v['median_ms'], v['min_ms'], v['max_ms'])


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('--out', default=None, help='write the figures as JSON')
    args = ap.parse_args()
    from acoustic_system import AcousticSystem
    from audio_models.ConvNets_SpeechCommands.models import create_model
    from dmad_hip.transforms import MelSpectrogramDB

    eng = E.Engine(max_batch=64, precision=E.FP32, with_wavenet=False)
    sd = synth.wideresnet28_10_state_dict(synth.WRN_SEED)
    wrn = create_model('wideresnet28_10', 10, 1)
    wrn.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()})
    wrn = wrn.cuda().eval().bind_engine(eng)
    system = AcousticSystem(classifier=wrn, transform=MelSpectrogramDB(eng, grad_backend='hip'), defender=None).eval()
    base = torch.from_numpy(np.stack([synth.synthetic_clip(i) for i in range(20)])).float().cuda()
    out = {'runs': RUNS, 'engine': 'FP32, max_batch 64', 'forward': {}, 'gradient': {}, 'memory': {}}
    spec_all = eng.mel_db(base.repeat(4, 1, 1).contiguous()).view(-1, 1, 32, 32)
    for B in FWD_BATCHES:
        spec = spec_all[:B].contiguous()
        fns = {'hip': lambda: eng.classify(spec), 'torch': lambda: wrn.torch_forward(spec)}
        ts = {b: [] for b in fns}
        with torch.no_grad():
            for b in fns:
                fns[b]()
            for _ in range(RUNS):
                for b in fns:
                    ts[b].append(timed(fns[b]))
        out['forward'][str(B)] = {b: stats(ts[b]) for b in ts}
    for B in BATCHES:
        x = base.repeat(B // 20, 1, 1).contiguous()
        with torch.no_grad():
            y = system(x).argmax(1)

        def grad(backend):
            wrn.grad_backend = backend
            xi = x.clone().requires_grad_(True)
            torch.nn.functional.cross_entropy(system(xi), y).backward()
            return xi.grad

        ts = {b: [] for b in ('hip', 'torch')}
        mem = {}
        for b in ts:
            grad(b)                                                       # warm-up: reservations, MIOpen's algorithm search
        for _ in range(RUNS):
            for b in ts:
                ts[b].append(timed(lambda: grad(b)))
        for b in ts:
            wrn.zero_grad(set_to_none=True)
            torch.cuda.synchronize()
            torch.cuda.reset_peak_memory_stats()
            before = torch.cuda.memory_allocated()
            grad(b)
            torch.cuda.synchronize()
            mem[b] = {'torch_peak_bytes': int(torch.cuda.max_memory_allocated()), 'torch_resident_before_bytes': int(before),
                      'engine_bytes': int(eng.device_bytes())}
        wrn.zero_grad(set_to_none=True)
        out['gradient'][str(B)] = {b: stats(ts[b]) for b in ts}
        out['memory'][str(B)] = mem
    wrn.grad_backend = 'auto'
    for name in ('forward', 'gradient'):
        print('| %s, B | hip median ms (min - max) | torch median ms (min - max) | torch / hip |\n|---|---|---|---|' % name)
        for B, v in out[name].items():
            print('| %s | %s | %s | %.2f |' % (B, row(v['hip']), row(v['torch']), v['torch']['median_ms'] / v['hip']['median_ms']))
        print()
    print('| B | backend | torch peak MB over one gradient | of which resident before it MB | engine MB (dmad_device_bytes) |\n|---|---|---|---|---|')
    for B, v in out['memory'].items():
        for b, m in v.items():
            print('| %s | %s | %.1f | %.1f | %.1f |' % (B, b, m['torch_peak_bytes'] / 1e6, m['torch_resident_before_bytes'] / 1e6, m['engine_bytes'] / 1e6))
    if args.out:
        with open(args.out, 'w') as f:
            json.dump(out, f, indent=1)
    eng.close()


if __name__ == '__main__':
    main()
