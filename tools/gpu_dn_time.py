"""Time and memory of DenseNet-BC-100-12 on the engine: the forward, one CW gradient through the engine's VJP against the torch branch, and
the bottleneck kernel against the general kernels it replaces.

  python tools/gpu_dn_time.py [--out FILE]      # one MI355X; prints the tables of profiles/r21_densenet.md

AcousticSystem(DenseNet, MelSpectrogramDB, None) over one FP32 engine (max_batch 64, the drivers' default) with the synthetic calibrated
DenseNet-BC-100-12 (seed 10012).  Every figure is the median of 7 timed runs after a warm-up, the two sides alternating; host clock around
a run that ends in a device synchronise; min - max beside it.
  * forward: dmad_classify on B = 1, 20, 64 and 4 020 spectrograms (4 020: one FAKEBOB estimate, chunked by max_batch inside the call)
    against the module's own layers under no_grad (MIOpen);
  * one CW gradient = forward plus backward of the cross-entropy through mel dB -> DenseNet, at B = 20 (the driver's batch) and B = 300
    (EOT 15 x 20), for grad_backend 'hip' (dmad_dn_vjp) and 'torch' (the module's own layers and a torch activation tape); the mel
    front-end is the engine's VJP in both;
  * memory: torch.cuda.max_memory_allocated over one gradient (reset before it) next to dmad_device_bytes after it;
  * one bottleneck layer (dense1's last: 204 -> 48 on 20 x 32 x 32 pixels): dmad_dn_pw against dmad_wrn_preact + dmad_conv_f32 on an image
    zero-padded to what gemm_f32 tiles (K 208, M 64), 50 calls back to back per timed run."""
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

BATCHES, FWD_BATCHES, RUNS, REPEAT = (20, 300), (1, 20, 64, 4020), 7, 50


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


def alternate(fns):
    ts = {b: [] for b in fns}
    for b in fns:
        fns[b]()
    for _ in range(RUNS):
        for b in fns:
            ts[b].append(timed(fns[b]))
    return {b: stats(ts[b]) for b in ts}


def bottleneck_pair():
    """dense1's last layer on 20 spectrograms: the fused kernel, and the pre-activation kernel + gemm_f32 on the zero-padded image"""
    gen = torch.Generator().manual_seed(5)
    n_px, cin, K, M = 20 * 1024, 204, 208, 64
    x = torch.zeros(n_px, 216)
    x[:, :cin] = torch.rand(n_px, cin, generator=gen) * 2 - 1
    w, s1, b1, s2, b2 = torch.rand(48, cin, generator=gen) - 0.5, torch.rand(cin, generator=gen) + 0.5, torch.rand(cin, generator=gen) - 0.5, \
        torch.rand(48, generator=gen) + 0.5, torch.rand(48, generator=gen) - 0.5
    xp, wp = torch.zeros(20, 32, 32, K), torch.zeros(1, 1, M, K)
    xp.view(n_px, K)[:, :cin], wp[0, 0, :48, :cin] = x[:, :cin], w
    pad = lambda v, n, fill: torch.cat([v, torch.full((n - v.numel(),), fill)])
    s1p, b1p, s2p, b2p = pad(s1, K, 1.0), pad(b1, K, 0.0), pad(s2, M, 1.0), pad(b2, M, 0.0)
    x, w, s1, b1, s2, b2, xp, wp, s1p, b1p, s2p, b2p = (t.cuda() for t in (x, w, s1, b1, s2, b2, xp, wp, s1p, b1p, s2p, b2p))
    fused = lambda: E.dn_pw(x, w, s1, b1, s2, b2)
    general = lambda: E.conv_f32(E.wrn_preact(xp, s1p, b1p), wp, shift=b2p, scale=s2p, relu=True)[0]
    a, b = fused(), general().view(n_px, M)[:, :48]
    err = float((a - b).abs().max() / b.abs().max())
    many = lambda fn: (lambda: [fn() for _ in range(REPEAT)])               # REPEAT launches per timed run: the host's launch cost overlaps the device's work
    out = alternate({'dn_pw': many(fused), 'wrn_preact + gemm_f32': many(general)})
    out['agreement_relmax'] = err
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('--out', default=None, help='write the figures as JSON')
    args = ap.parse_args()
    from acoustic_system import AcousticSystem
    from audio_models.ConvNets_SpeechCommands.models import DenseNet
    from dmad_hip.transforms import MelSpectrogramDB

    eng = E.Engine(max_batch=64, precision=E.FP32, with_wavenet=False)
    sd = synth.densenet_bc_100_12_state_dict(synth.DN_SEED)
    net = DenseNet(depth=100, growthRate=12, compressionRate=2, num_classes=10, in_channels=1)
    net.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()})
    net = net.cuda().eval().bind_engine(eng)
    system = AcousticSystem(classifier=net, transform=MelSpectrogramDB(eng, grad_backend='hip'), defender=None).eval()
    base = torch.from_numpy(np.stack([synth.synthetic_clip(i) for i in range(20)])).float().cuda()
    out = {'runs': RUNS, 'engine': 'FP32, max_batch 64', 'forward': {}, 'gradient': {}, 'memory': {}}
    spec_all = eng.mel_db(base).view(-1, 1, 32, 32).repeat(201, 1, 1, 1).contiguous()
    for B in FWD_BATCHES:
        spec = spec_all[:B].contiguous()
        with torch.no_grad():
            out['forward'][str(B)] = alternate({'hip': lambda: eng.classify(spec), 'torch': lambda: net.torch_forward(spec)})
        print('forward B = %d done' % B, file=sys.stderr, flush=True)
    for B in BATCHES:
        x = base.repeat(B // 20, 1, 1).contiguous()
        with torch.no_grad():
            y = system(x).argmax(1)

        def grad(backend):
            net.grad_backend = backend
            xi = x.clone().requires_grad_(True)
            torch.nn.functional.cross_entropy(system(xi), y).backward()
            return xi.grad

        out['gradient'][str(B)] = alternate({'hip': lambda: grad('hip'), 'torch': lambda: grad('torch')})
        print('gradient B = %d done' % B, file=sys.stderr, flush=True)
        mem = {}
        for b in ('hip', 'torch'):
            net.zero_grad(set_to_none=True)
            torch.cuda.synchronize()
            torch.cuda.reset_peak_memory_stats()
            before = torch.cuda.memory_allocated()
            grad(b)
            torch.cuda.synchronize()
            mem[b] = {'torch_peak_bytes': int(torch.cuda.max_memory_allocated()), 'torch_resident_before_bytes': int(before),
                      'engine_bytes': int(eng.device_bytes())}
        net.zero_grad(set_to_none=True)
        out['memory'][str(B)] = mem
    net.grad_backend = 'auto'
    out['bottleneck'] = bottleneck_pair()
    for name in ('forward', 'gradient'):
        print('| %s, B | hip median ms (min - max) | torch median ms (min - max) | torch / hip |\n|---|---|---|---|' % name)
        for B, v in out[name].items():
            print('| %s | %s | %s | %.2f |' % (B, row(v['hip']), row(v['torch']), v['torch']['median_ms'] / v['hip']['median_ms']))
        print()
    print('| B | backend | torch peak MB over one gradient | of which resident before it MB | engine MB (dmad_device_bytes) |\n|---|---|---|---|---|')
    for B, v in out['memory'].items():
        for b, m in v.items():
            print('| %s | %s | %.1f | %.1f | %.1f |' % (B, b, m['torch_peak_bytes'] / 1e6, m['torch_resident_before_bytes'] / 1e6, m['engine_bytes'] / 1e6))
    bp = out['bottleneck']
    print('\n| 204 -> 48 on 20 480 pixels, %d calls back to back | median us per call (min - max) |\n|---|---|' % REPEAT)
    for k in ('dn_pw', 'wrn_preact + gemm_f32'):
        print('| %s | %.1f (%.1f - %.1f) |' % ((k,) + tuple(1e3 * bp[k][f] / REPEAT for f in ('median_ms', 'min_ms', 'max_ms'))))
    print('agreement of the two: relmax %.2e' % bp['agreement_relmax'])
    if args.out:
        with open(args.out, 'w') as f:
            json.dump(out, f, indent=1)
    eng.close()


if __name__ == '__main__':
    main()
