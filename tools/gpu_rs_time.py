"""Time and memory of one RobustCertificate.smooth_predict without a denoiser (the plain randomized-smoothing baseline, the driver's
--defense_method randsmooth): the fused route (dmad_rs_smooth_votes / dmad_m5_rs_smooth_votes) against the host loop on the same commit.

  python tools/gpu_rs_time.py [--out FILE] [--runs 7] [--big-runs 7] [--nets vgg19_bn,resnext29,m5]   # the tables of profiles/r22_randsmooth.md
  python tools/gpu_rs_time.py --kernels 20      # 20 full passes of either form and nothing else: run it under rocprofv3 --kernel-trace --stats

One FP32 engine per classifier (max_batch 64, the drivers' default, no WaveNet): synthetic VGG19_bn and ResNeXt29 (the driver's default
classifier) behind MelSpectrogramDB, and M5 (the trained kernel_size = 160 checkpoint of tests/golden/m5_k160_state.npz) after
use_engine() with no transform.  The baseline is the same RobustCertificate with _fused_rs() switched off, i.e. _generic_votes, which is
what the parent commit ran: per batch_size rows x.repeat, dmad_philox_normal, a torch multiply and add, the mel front-end, the classifier
and dmad_vote.
  * N = 10 000 at the driver's batch_size 16, both routes; N = 100 000, the fused route only; synthetic clip 0, sigma 0.5, one seed;
  * time: one warm-up run each, then --runs timed runs each, the routes alternating; host clock around a smooth_predict (it ends in the
    copy of the counts to the host); the table gives the median and the min - max spread;
  * memory: torch.cuda.max_memory_allocated over one run (reset before it) less what was resident before it; the engines' own
    workspaces (dmad_device_bytes) are resident before either route and printed beside the table."""
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

N_SMALL, N_BIG, BATCH_SIZE, SIGMA, MAX_BATCH = 10000, 100000, 16, 0.5, 64


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0


def stats(ts):
    return {'median_ms': 1e3 * float(np.median(ts)), 'min_ms': 1e3 * min(ts), 'max_ms': 1e3 * max(ts)}


def measure(fns, runs):
    """{name: fn} -> ({name: time stats}, {name: bytes torch allocated on top of what was resident})"""
    ts = {k: [] for k in fns}
    for k in fns:
        fns[k]()
    for _ in range(runs):
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


def build(net):
    """(engine, classifier module, transform) of one row of the table"""
    from dmad_hip.transforms import MelSpectrogramDB
    if net == 'm5':
        from audio_models.M5.M5Net import M5
        eng = E.Engine(max_batch=MAX_BATCH, precision=E.FP32, with_wavenet=False, with_classifier=False)
        with np.load(os.path.join(ROOT, 'tests', 'golden', 'm5_k160_state.npz')) as z:
            sd = {k: torch.from_numpy(z[k]) for k in z.files}
        m = M5(n_input=1, first_kernel_size=160, n_output=10)
        m.load_state_dict(sd)
        return eng, m.cuda().eval().use_engine(eng), None
    eng = E.Engine(max_batch=MAX_BATCH, precision=E.FP32, with_wavenet=False)
    if net == 'vgg19_bn':
        from audio_models.ConvNets_SpeechCommands.models.vgg import vgg19_bn
        m, sd = vgg19_bn(num_classes=10, in_channels=1), synth.vgg19_bn_state_dict(4321)
    else:
        from audio_models.ConvNets_SpeechCommands.models.resnext import CifarResNeXt
        m, sd = CifarResNeXt(nlabels=10, in_channels=1), synth.resnext29_state_dict(2929)
    m.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()})
    return eng, m.eval().bind_engine(eng), MelSpectrogramDB(eng)


def certificates(net):
    from robustness_eval.certified_robust import RobustCertificate

    class HostLoop(RobustCertificate):
        def _fused_rs(self):
            return None

    eng, m, tr = build(net)
    fused, host = RobustCertificate(m, tr, None, seed=3), HostLoop(m, tr, None, seed=3)
    assert fused._fused_rs() is not None, 'the fused route does not apply to %s' % net
    return eng, fused, host


def kernels_only(passes):
    """`passes` full passes of the fused form and of the host loop's form on VGG19_bn, for a kernel trace"""
    eng, fused, host = certificates('vgg19_bn')
    x = torch.from_numpy(synth.synthetic_clip(0)).float().reshape(1, -1).cuda()
    for rc in (fused, host):
        rc.smooth_predict(x, MAX_BATCH * passes, SIGMA, MAX_BATCH)
    torch.cuda.synchronize()
    eng.close()


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('--out', default=None, help='write the figures as JSON (rewritten after every cell)')
    ap.add_argument('--runs', type=int, default=7)
    ap.add_argument('--big-runs', type=int, default=7, help='timed runs of the N = 100 000 cells')
    ap.add_argument('--nets', default='vgg19_bn,resnext29,m5')
    ap.add_argument('--kernels', type=int, default=0, help='only run this many full passes of either form (for rocprofv3)')
    args = ap.parse_args()
    if args.kernels:
        return kernels_only(args.kernels)
    x = torch.from_numpy(synth.synthetic_clip(0)).float().reshape(1, -1).cuda()
    out = {'runs': args.runs, 'big_runs': args.big_runs, 'engine': 'FP32, max_batch %d, with_wavenet 0' % MAX_BATCH, 'sigma': SIGMA,
           'batch_size': BATCH_SIZE, 'cells': {}}
    print('| net | N | host loop median ms (min - max) | fused median ms (min - max) | host / fused | host MB allocated | fused MB allocated |\n'
          '|---|---|---|---|---|---|---|', flush=True)
    for net in args.nets.split(','):
        eng, fused, host = certificates(net)
        same = [rc.smooth_predict(x, 256, SIGMA, BATCH_SIZE).tolist() for rc in (fused, host)]
        assert same[0] == same[1], same
        t, m = measure({k: (lambda rc=rc: rc.smooth_predict(x, N_SMALL, SIGMA, BATCH_SIZE)) for k, rc in (('fused', fused), ('host', host))}, args.runs)
        out['cells']['%s/%d' % (net, N_SMALL)] = {'time': t, 'bytes': m, 'engine_bytes': eng.device_bytes()}
        f, h = t['fused'], t['host']
        slower = '**' if f['median_ms'] > h['median_ms'] else ''
        print('| %s | %d | %.1f (%.1f - %.1f) | %s%.1f (%.1f - %.1f)%s | %.2f | %.1f | %.1f |'
              % (net, N_SMALL, h['median_ms'], h['min_ms'], h['max_ms'], slower, f['median_ms'], f['min_ms'], f['max_ms'], slower,
                 h['median_ms'] / f['median_ms'], m['host'] / 1e6, m['fused'] / 1e6), flush=True)
        t, m = measure({'fused': lambda: fused.smooth_predict(x, N_BIG, SIGMA, BATCH_SIZE)}, args.big_runs)
        out['cells']['%s/%d' % (net, N_BIG)] = {'time': t, 'bytes': m, 'engine_bytes': eng.device_bytes()}
        f = t['fused']
        print('| %s | %d | - | %.1f (%.1f - %.1f) | - | - | %.1f |' % (net, N_BIG, f['median_ms'], f['min_ms'], f['max_ms'], m['fused'] / 1e6), flush=True)
        print('| %s engine MB (dmad_device_bytes) | %.1f | | | | | |' % (net, eng.device_bytes() / 1e6), flush=True)
        if args.out:
            with open(args.out, 'w') as fo:
                json.dump(out, fo, indent=1)
        eng.close()


if __name__ == '__main__':
    main()
