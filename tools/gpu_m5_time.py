"""Time and memory of the M5 waveform classifier: the engine (dmad_m5_logits / dmad_m5_vjp) against the torch module's own layers on the
same commit.

  python tools/gpu_m5_time.py [--out FILE]      # one MI355X; prints the tables of profiles/r15_m5.md

AcousticSystem(M5, None, None) over one FP32 engine (max_batch 64, the drivers' default, no WaveNet) with the trained kernel_size = 160
checkpoint of tests/golden/m5_k160_state.npz; the torch side is the same module with no engine in use (a default M5: about twenty
framework launches per pass and a full activation tape), in the same process.
  * forward: 4 020 rows, one FAKEBOB estimate (20 clips x 201 probes), under no_grad;
  * gradient: forward plus backward of the cross-entropy at B = 20 (the driver's batch) and B = 300 (EOT 15 x 20), M5.grad_backend 'hip'
    against the layers;
  * time: one warm-up run each, then 7 timed runs each, the two sides alternating; host clock around a run that ends in a device
    synchronise; the table gives the median and the min - max spread;
  * memory: torch.cuda.max_memory_allocated over one run (reset before it) less what was resident before it.  The engine has no
    workspace for M5: its side allocates the results and nothing else."""
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

FORWARD_ROWS, BATCHES, RUNS = 4020, (20, 300), 7


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0


def stats(ts):
    return {'median_ms': 1e3 * float(np.median(ts)), 'min_ms': 1e3 * min(ts), 'max_ms': 1e3 * max(ts)}


def measure(fns):
    """{name: fn} -> ({name: time stats}, {name: bytes torch allocated on top of what was resident})"""
    ts = {k: [] for k in fns}
    for k in fns:
        fns[k]()                                                          # warm-up: MIOpen's algorithm search, the allocator's pools
    for _ in range(RUNS):
        for k in fns:
            ts[k].append(timed(fns[k]))
    mem = {}
    for k in fns:
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        before = torch.cuda.memory_allocated()
        fns[k]()
        torch.cuda.synchronize()
        mem[k] = int(torch.cuda.max_memory_allocated() - before)
    return {k: stats(v) for k, v in ts.items()}, mem


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('--out', default=None, help='write the figures as JSON')
    args = ap.parse_args()
    from acoustic_system import AcousticSystem
    from audio_models.M5.M5Net import M5

    with np.load(os.path.join(ROOT, 'tests', 'golden', 'm5_k160_state.npz')) as z:
        sd = {k: torch.from_numpy(z[k]) for k in z.files}

    def module():
        m = M5(n_input=1, first_kernel_size=160, n_output=10)
        m.load_state_dict(sd)
        return m.cuda().eval()

    eng = E.Engine(max_batch=64, precision=E.FP32, with_wavenet=False)
    hip = module().use_engine(eng)
    hip.grad_backend = 'hip'
    systems = {'hip': AcousticSystem(hip, None, None).eval(), 'torch': AcousticSystem(module(), None, None).eval()}
    base = torch.from_numpy(np.stack([synth.synthetic_clip(i) for i in range(20)])).float().cuda()
    out = {'runs': RUNS, 'engine': 'FP32, max_batch 64, with_wavenet 0', 'forward': {}, 'gradient': {}}

    x = base.repeat(FORWARD_ROWS // 20, 1, 1).contiguous()

    def forward(system):
        with torch.no_grad():
            return system(x)

    t, m = measure({k: (lambda s=s: forward(s)) for k, s in systems.items()})
    out['forward'][str(FORWARD_ROWS)] = {'time': t, 'bytes': m}
    for B in BATCHES:
        xb = base.repeat(B // 20, 1, 1).contiguous()
        with torch.no_grad():
            y = systems['torch'](xb).argmax(1)

        def grad(system):
            xi = xb.clone().requires_grad_(True)
            torch.nn.functional.cross_entropy(system(xi), y).backward()
            system.zero_grad(set_to_none=True)
            return xi.grad

        t, m = measure({k: (lambda s=s: grad(s)) for k, s in systems.items()})
        out['gradient'][str(B)] = {'time': t, 'bytes': m}
    for what in ('forward', 'gradient'):
        print('\n| %s rows | hip median ms (min - max) | torch median ms (min - max) | torch / hip | hip MB allocated | torch MB allocated |\n'
              '|---|---|---|---|---|---|' % what)
        for B, v in out[what].items():
            h, t = v['time']['hip'], v['time']['torch']
            print('| %s | %.3f (%.3f - %.3f) | %.3f (%.3f - %.3f) | %.2f | %.1f | %.1f |'
                  % (B, h['median_ms'], h['min_ms'], h['max_ms'], t['median_ms'], t['min_ms'], t['max_ms'], t['median_ms'] / h['median_ms'],
                     v['bytes']['hip'] / 1e6, v['bytes']['torch'] / 1e6))
    print('\nengine MB (dmad_device_bytes): %.1f' % (eng.device_bytes() / 1e6))
    if args.out:
        with open(args.out, 'w') as f:
            json.dump(out, f, indent=1)
    eng.close()


if __name__ == '__main__':
    main()
