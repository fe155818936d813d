"""Time and memory of one CW gradient through the VGG19_bn classifier: the engine's VJP against the torch branch of the same commit.

  python tools/gpu_vgg_vjp_time.py [--out FILE]      # one MI355X; prints the tables of profiles/r14_vgg_vjp.md

AcousticSystem(VGG, MelSpectrogramDB, None) over one FP32 engine (max_batch 64, the drivers' default) with the synthetic calibrated
VGG19_bn (seed 4321).  One CW gradient = forward plus backward of the cross-entropy through mel dB -> VGG19_bn, at B = 20 (the driver's
batch) and B = 300 (EOT 15 x 20), for VGG.grad_backend 'hip' (dmad_vgg_vjp) and 'torch' (the module's own layers: MIOpen convolutions
and a torch activation tape) in the same process; the mel front-end is the engine's VJP in both, only the classifier differs.
  * time: one warm-up run each, then 7 timed runs each, the two backends alternating; host clock around a run that ends in a device
    synchronise; the table gives the median and the min - max spread;
  * memory: torch.cuda.max_memory_allocated over one gradient (reset before it) next to dmad_device_bytes after it.  The engine's
    figure holds everything the engine owns (weights, work maps, every VJP reservation), the torch figure only what torch allocated on
    top: the module's parameters, the activations and MIOpen's workspaces;
  * the pool + ReLU backward kernel alone on the B = 300 maps, device events around 20 launches, with the effective GB/s (y and gpre of
    the full map, g of a quarter: 2.25 maps of 4-byte values moved) against the 8 TB/s of HBM."""
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

BATCHES, RUNS = (20, 300), 7
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
    from audio_models.ConvNets_SpeechCommands.models.vgg import vgg19_bn
    from dmad_hip.transforms import MelSpectrogramDB

    eng = E.Engine(max_batch=64, precision=E.FP32, with_wavenet=False)
    sd = synth.vgg19_bn_state_dict(4321)
    vgg = vgg19_bn(num_classes=10, in_channels=1)
    vgg.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()})
    vgg = vgg.cuda().eval().bind_engine(eng)
    system = AcousticSystem(classifier=vgg, transform=MelSpectrogramDB(eng, grad_backend='hip'), defender=None).eval()
    base = torch.from_numpy(np.stack([synth.synthetic_clip(i) for i in range(20)])).float().cuda()
    out = {'runs': RUNS, 'engine': 'FP32, max_batch 64', 'gradient': {}, 'memory': {}, 'pool_relu_bwd': {}}
    for B in BATCHES:
        x = base.repeat(B // 20, 1, 1).contiguous()
        with torch.no_grad():
            y = system(x).argmax(1)

        def grad(backend):
            vgg.grad_backend = backend
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
            vgg.zero_grad(set_to_none=True)
            torch.cuda.synchronize()
            torch.cuda.reset_peak_memory_stats()
            before = torch.cuda.memory_allocated()
            grad(b)
            torch.cuda.synchronize()
            mem[b] = {'torch_peak_bytes': int(torch.cuda.max_memory_allocated()), 'torch_resident_before_bytes': int(before),
                      'engine_bytes': int(eng.device_bytes())}
        vgg.zero_grad(set_to_none=True)
        out['gradient'][str(B)] = {b: stats(ts[b]) for b in ts}
        out['memory'][str(B)] = mem
    vgg.grad_backend = 'auto'
    Bp = BATCHES[-1]
    for H, C in ((32, 64), (16, 128), (8, 256), (4, 512), (2, 512)):
        yv = torch.relu(torch.randn(Bp, H, H, C, device='cuda'))
        gv = torch.randn(Bp, H // 2, H // 2, C, device='cuda')
        E.vgg_pool_relu_bwd(gv, yv)
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        for _ in range(20):
            E.vgg_pool_relu_bwd(gv, yv)
        t1.record()
        torch.cuda.synchronize()
        ms = t0.elapsed_time(t1) / 20
        gbs = 2.25 * yv.numel() * 4 / (ms * 1e-3) / 1e9
        out['pool_relu_bwd']['%dx%dx%d' % (H, H, C)] = {'ms': ms, 'mbytes': 2.25 * yv.numel() * 4 / 1e6, 'gbs': gbs, 'hbm_share': gbs / HBM_GBS}
    print('| B | hip median ms (min - max) | torch median ms (min - max) | torch / hip |\n|---|---|---|---|')
    for B, v in out['gradient'].items():
        h, t = v['hip'], v['torch']
        print('| %s | %.2f (%.2f - %.2f) | %.2f (%.2f - %.2f) | %.2f |' % (B, h['median_ms'], h['min_ms'], h['max_ms'], t['median_ms'], t['min_ms'],
                                                                         t['max_ms'], t['median_ms'] / h['median_ms']))
    print('\n| B | backend | torch peak MB over one gradient | of which resident before it MB | engine MB (dmad_device_bytes) |\n|---|---|---|---|---|')
    for B, v in out['memory'].items():
        for b, m in v.items():
            print('| %s | %s | %.1f | %.1f | %.1f |' % (B, b, m['torch_peak_bytes'] / 1e6, m['torch_resident_before_bytes'] / 1e6, m['engine_bytes'] / 1e6))
    print('\n| pool + ReLU backward, B = %d | ms per launch | MB moved | GB/s | of 8 TB/s |\n|---|---|---|---|---|' % Bp)
    for k, s in out['pool_relu_bwd'].items():
        print('| %s | %.4f | %.1f | %.0f | %.1f %% |' % (k, s['ms'], s['mbytes'], s['gbs'], 100 * s['hbm_share']))
    if args.out:
        with open(args.out, 'w') as f:
            json.dump(out, f, indent=1)
    eng.close()


if __name__ == '__main__':
    main()
