"""Time and memory of one stage-2 iteration of the imperceptible attack (Qin-I): the engine's masking step against the torch branch.

  python tools/gpu_qin_time.py [--out FILE]      # one MI355X; prints the tables of profiles/r16_qin.md

AcousticSystem(ResNeXt29, MelSpectrogramDB, None) over one FP32 engine (max_batch 64, the drivers' default) with the synthetic
ResNeXt29 (seed 2929), both gradients of the network on the engine's VJPs, B = 20 (the driver's batch), theta and psd_scale from the
host masker, delta = 65 / 32768 times random signs.  One stage-2 iteration = the network part (forward, cross-entropy, backward:
the same in every case) plus the masking part, which is timed in three forms:
  * hip            one Engine.masking_step call (STFT GEMM, hinge, transposed GEMM, overlap-add with the update) and the B losses;
  * torch          AudioAttack._loss_gradient_masking_threshold on masking_backend='torch' (torch.stft with autograd, the hinge in
                   float64), the update as tensor operations, and the B losses;
  * torch + host   the same with the reference's per-iteration round trip reinstated (white_box_attack.py l.628-629: delta to the
                   host as numpy, padded there, and back) — a switch of this tool only, the package does not make that trip.
Time: one warm-up run each, then 7 timed runs each, the three forms alternating; a run is 10 iterations between two device
synchronisations on the host clock; the tables give the median per iteration and the min - max spread.  Memory: the bytes torch
allocates over one iteration (the growth of allocated_bytes.all.allocated) and its peak above what was resident before it."""
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

B, RUNS, ITERS = 20, 7, 10
FORMS = ('hip', 'torch', 'torch + host')


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(ITERS):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / ITERS


def stats(ts):
    return {'median_ms': 1e3 * float(np.median(ts)), 'min_ms': 1e3 * min(ts), 'max_ms': 1e3 * max(ts)}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('--out', default=None, help='write the figures as JSON')
    args = ap.parse_args()
    from acoustic_system import AcousticSystem
    from audio_models.ConvNets_SpeechCommands.models.resnext import CifarResNeXt
    from dmad_hip.transforms import MelSpectrogramDB
    from robustness_eval.white_box_attack import AudioAttack, PsychoacousticMasker

    eng = E.Engine(max_batch=64, precision=E.FP32, with_wavenet=False)
    rx = CifarResNeXt(nlabels=10, in_channels=1)
    rx.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in synth.resnext29_state_dict(2929).items()})
    rx = rx.cuda().eval().bind_engine(eng)
    rx.grad_backend = 'hip'
    eng.reserve_classifier_vjp(B)
    system = AcousticSystem(classifier=rx, transform=MelSpectrogramDB(eng, grad_backend='hip'), defender=None).eval()
    x = torch.from_numpy(np.stack([synth.synthetic_clip(i) for i in range(B)])).float().cuda()
    with torch.no_grad():
        y = system(x).argmax(1)
    att = {b: AudioAttack(system, masker=PsychoacousticMasker(), eot_attack_size=1, eot_defense_size=1, verbose=0, masking_backend=b)
           for b in ('hip', 'torch')}
    t0 = time.perf_counter()
    theta, psd_max = att['torch']._stabilized_threshold_and_psd_maximum(x)
    masker_s = time.perf_counter() - t0
    theta32, scale32 = theta.float(), (pow(10.0, 9.6) / psd_max).float()
    rng = np.random.RandomState(0)
    delta0 = torch.from_numpy((65.0 / 32768.0) * (rng.randint(0, 2, (B, 1, 16000)) * 2.0 - 1.0)).float().cuda()
    alpha = torch.full((B, 1, 1), 0.05, device='cuda')
    lr = -2.0 ** -15
    state = {'delta': delta0.clone().requires_grad_(True), 'g_net': torch.zeros_like(delta0)}

    def network():
        d = state['delta']
        d.grad = None
        torch.nn.functional.cross_entropy(system(x + d), y).backward()
        state['g_net'] = d.grad.data

    def masking(form):
        d, g_net = state['delta'], state['g_net']
        if form == 'hip':
            return eng.masking_step(x, d.data, g_net, alpha, lr, theta32, scale32).tolist()
        p = d
        if form == 'torch + host':                                        # the reference's round trip, l.628-629
            host = d.detach().cpu().numpy()[:, 0]
            padded = np.zeros(host.shape, dtype=host.dtype)
            padded[:] = host
            p = torch.from_numpy(padded).to(x.device)
        g_theta, loss = att['torch']._loss_gradient_masking_threshold(p, x, theta, psd_max)
        d.data = d.data + lr * (g_net + alpha * g_theta)
        d.data = (x + d.data).clamp(-1, 1) - x
        return loss.tolist()

    def iteration(form):
        network()
        return masking(form)

    out = {'batch': B, 'runs': RUNS, 'iterations_per_run': ITERS, 'engine': 'FP32, max_batch 64', 'masker_host_s_per_batch': masker_s,
           'network': {}, 'masking': {}, 'iteration': {}, 'memory': {}}
    network()
    ts = [timed(network) for _ in range(RUNS)]
    out['network'] = stats(ts)
    for what, fn in (('masking', masking), ('iteration', iteration)):
        t = {f: [] for f in FORMS}
        for f in FORMS:
            state['delta'].data.copy_(delta0)
            fn(f)                                                          # warm-up: the VJP workspace, the FFT plans
        for _ in range(RUNS):
            for f in FORMS:
                state['delta'].data.copy_(delta0)
                t[f].append(timed(lambda: fn(f)))
        out[what] = {f: stats(t[f]) for f in FORMS}
    for f in FORMS:
        state['delta'].data.copy_(delta0)
        iteration(f)
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        before, alloc0 = torch.cuda.memory_allocated(), torch.cuda.memory_stats()['allocated_bytes.all.allocated']
        iteration(f)
        torch.cuda.synchronize()
        out['memory'][f] = {'allocated_bytes': int(torch.cuda.memory_stats()['allocated_bytes.all.allocated'] - alloc0),
                            'peak_above_resident_bytes': int(torch.cuda.max_memory_allocated() - before),
                            'engine_bytes': int(eng.device_bytes())}
    n = out['network']
    print('host masker: %.2f s per batch of %d clips (once per batch)\n' % (masker_s, B))
    print('network part (forward, cross-entropy, backward), B = %d: %.2f ms (%.2f - %.2f)\n' % (B, n['median_ms'], n['min_ms'], n['max_ms']))
    print('| form | masking part median ms (min - max) | whole iteration median ms (min - max) | iteration / hip |\n|---|---|---|---|')
    h = out['iteration']['hip']['median_ms']
    for f in FORMS:
        m, i = out['masking'][f], out['iteration'][f]
        print('| %s | %.3f (%.3f - %.3f) | %.2f (%.2f - %.2f) | %.2f |' % (f, m['median_ms'], m['min_ms'], m['max_ms'], i['median_ms'], i['min_ms'],
                                                                           i['max_ms'], i['median_ms'] / h))
    print('\n| form | MB torch allocates over one iteration | peak MB above the resident | engine MB (dmad_device_bytes) |\n|---|---|---|---|')
    for f in FORMS:
        m = out['memory'][f]
        print('| %s | %.1f | %.1f | %.1f |' % (f, m['allocated_bytes'] / 1e6, m['peak_above_resident_bytes'] / 1e6, m['engine_bytes'] / 1e6))
    if args.out:
        with open(args.out, 'w') as f:
            json.dump(out, f, indent=1)
    eng.close()


if __name__ == '__main__':
    main()
