"""Time the classifier-side VJPs (dmad_classify_vjp, dmad_mel_db_vjp) against the torch branch, and one AudioAttack iteration.

  python tools/gpu_classifier_vjp_time.py            # one MI355X; prints a table for profiles/r10_classifier_vjp.md

Per spectrogram at B = 20 (the driver's batch) and B = 64: the engine's fp32 ResNeXt29 forward, the HIP VJP (recomputed forward +
backward), the torch branch's forward + backward (CifarResNeXt's own layers, MIOpen), the HIP mel VJP and the torch mel branch; then
one stage-1 AudioAttack iteration (forward + loss.backward) of the whole system with --defense None and with RevDiffWave at t = 1,
hip and torch classifier / mel.  Synthetic calibrated ResNeXt29 (seed 2929) and WaveNet (seed 1234); medians of 5 after a warm-up."""
import json
import os
import sys
import tempfile
import time
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, 'diffusion-model-for-audio-defense_amd'), ROOT]

from dmad_hip import engine as E, synth  # noqa: E402

PEAK = 157.3e12                 # fp32 matrix, spec
RX_FLOP = 10.8e9                # one ResNeXt29 forward on 1 x 32 x 32 (5.39 GMAC)


def med(fn, reps=5):
    fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append(time.perf_counter() - t0)
    return float(np.median(ts))


def main():
    from audio_models.ConvNets_SpeechCommands.models.resnext import CifarResNeXt
    from dmad_hip.transforms import MelSpectrogramDB
    sd = synth.resnext29_state_dict(2929)
    wsd = synth.wavenet_state_dict(1234)
    eng = E.Engine(max_batch=64, precision=E.FP32)
    eng.load_wavenet(wsd)
    eng.load_resnext29(sd)
    rx = CifarResNeXt(nlabels=10, in_channels=1)
    rx.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()})
    rx = rx.cuda().eval().bind_engine(eng)
    rows = []
    for B in (20, 64):
        clips = torch.from_numpy(np.stack([synth.synthetic_clip(i % 16).reshape(-1) for i in range(B)])).float().unsqueeze(1).cuda()
        spec = eng.mel_db(clips)
        g = torch.randn(B, 10, device='cuda')
        gs = torch.randn(B, 1, 32, 32, device='cuda')
        before = eng.device_bytes()
        eng.reserve_classifier_vjp(B)
        grow = eng.device_bytes() - before
        t_fwd = med(lambda: eng.classify_tier(spec, 0))
        t_vjp = med(lambda: eng.classify_vjp(spec, g))
        rx.grad_backend = 'torch'

        def torch_cls():
            x = spec.clone().requires_grad_(True)
            torch.autograd.grad((rx(x) * g).sum(), x)
        t_tc = med(torch_cls)
        t_mel = med(lambda: eng.mel_db_vjp(clips, gs))

        def torch_mel():
            x = clips.clone().requires_grad_(True)
            torch.autograd.grad((MelSpectrogramDB(eng, grad_backend='torch')(x) * gs).sum(), x)
        t_tm = med(torch_mel)
        rows.append(dict(B=B, fwd_ms=1e3 * t_fwd / B, vjp_ms=1e3 * t_vjp / B, torch_cls_ms=1e3 * t_tc / B, mel_vjp_ms=1e3 * t_mel / B,
                         torch_mel_ms=1e3 * t_tm / B, vjp_peak=2 * RX_FLOP * B / t_vjp / PEAK, workspace_MB=grow / 2 ** 20))
    # one attack iteration of the whole system
    from acoustic_system import AcousticSystem
    from diffusion_models.diffwave_sde import RevDiffWave
    cfg = os.path.join(tempfile.mkdtemp(), 'config.json')
    with open(cfg, 'w') as f:
        json.dump({'diffusion_config': synth.DIFFUSION_CONFIG, 'wavenet_config': synth.WAVENET_CONFIG}, f)
    args = types.SimpleNamespace(ddpm_path=None, ddpm_config=cfg, t=1, score_type='guided_diffusion', sample_step=1, rand_t=False, t_delta=0,
                                 use_bm=False)
    den = RevDiffWave(args, state_dict=wsd, engine=eng, score_grad='hip', seed=0)
    B = 20
    x0 = torch.from_numpy(np.stack([synth.synthetic_clip(i).reshape(-1) for i in range(B)])).float().unsqueeze(1).cuda()
    y = torch.arange(B, device='cuda') % 10
    att = []
    for defense in ('None', 'Diffusion'):
        for backend in ('hip', 'torch'):
            rx.grad_backend = backend
            system = AcousticSystem(classifier=rx, transform=MelSpectrogramDB(eng, grad_backend=backend),
                                    defender=den if defense == 'Diffusion' else None, defense_type='wave')

            def it():
                d = torch.zeros_like(x0, requires_grad=True)
                torch.nn.functional.cross_entropy(system(x0 + d), y).backward()
            att.append(dict(defense=defense, backend=backend, ms=1e3 * med(it)))
    rx.grad_backend = 'auto'
    print('| B | fp32 forward, ms / spec | HIP VJP, ms / spec | torch branch fwd + bwd, ms / spec | HIP mel VJP, ms / clip | torch mel '
          'fwd + bwd, ms / clip | VJP share of fp32 peak (2 x forward FLOP) | workspace at reservation, MB |')
    print('|---|---|---|---|---|---|---|---|')
    for r in rows:
        print('| %d | %.3f | %.3f | %.3f | %.3f | %.3f | %.2f | %.0f |' % (r['B'], r['fwd_ms'], r['vjp_ms'], r['torch_cls_ms'], r['mel_vjp_ms'],
                                                                      r['torch_mel_ms'], r['vjp_peak'], r['workspace_MB']))
    print()
    print('| defense | classifier / mel gradient | one attack iteration at B = 20, ms |')
    print('|---|---|---|')
    for a in att:
        print('| %s | %s | %.1f |' % (a['defense'], a['backend'], a['ms']))
    eng.close()


if __name__ == '__main__':
    main()
