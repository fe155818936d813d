#!/usr/bin/env python3
"""Time the any-length exact-fp32 DiffWave path (profiles/r24_wavenet_len.md) on one MI355X: FP32 engine, full 36 x 12 geometry,
clip_len 32000, B = 1, synthetic weights, step t = 40, HIP events after a warm-up, medians of REPS = 7 runs.

  eps     wavenet_eps_len and wavenet_eps_vjp_len at len 8000 / 16000 / 24000 / 32000: ms and ms per 1000 samples
  clear   the cost of the padding invariant: a call at 8000 right after one at 32000 (the band [8000, 32000) of every map is cleared
          first) against a call at 8000 after another at 8000 (nothing is cleared), for eps and for the VJP
  cw      one CW iteration of the keyword-spotting driver's native-length Diffusion row at t = 1 on a 16000-sample clip (forward through
          purifier -> mel front-end -> keyword spotter with gradient, loss.backward(), signed step), --grad_backend hip against torch,
          with the growth of torch's allocator for both (the engine's own workspace is outside it: dmad_device_bytes is printed too)

Without an argument every step runs in a child process of its own under its own time limit, and prints one JSON line."""
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STEPS = {'eps': 240, 'clear': 180, 'cw': 300}           # seconds
REPS, T, CLIP = int(os.environ.get('REPS', 7)), 40, 32000
LENS = (8000, 16000, 24000, 32000)


def median(v):
    return sorted(v)[len(v) // 2]


def main(step):
    import torch
    sys.path[:0] = [ROOT, os.path.join(ROOT, 'diffusion-model-for-audio-defense_amd')]
    from dmad_hip import engine as E, synth

    def timed(fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        return a.elapsed_time(b)

    def rand(n, seed, scale=0.3):
        return torch.randn(1, n, device='cuda', generator=torch.Generator('cuda').manual_seed(seed)) * scale

    sd = synth.wavenet_state_dict(1234)
    eng = E.Engine(clip_len=CLIP, max_batch=1, precision=E.FP32, with_classifier=False)
    eng.load_wavenet(sd)
    out = {'step': step, 'reps': REPS, 'clip_len': CLIP}
    if step == 'eps':
        eng.reserve_vjp(1)
        for n in LENS:
            x, g = rand(n, n), rand(n, n + 1, 1.0)
            eng.wavenet_eps_len(x, T), eng.wavenet_eps_vjp_len(x, T, g)                     # warm-up (and the one clearing of this length)
            ms_e = median([timed(lambda: eng.wavenet_eps_len(x, T)) for _ in range(REPS)])
            ms_v = median([timed(lambda: eng.wavenet_eps_vjp_len(x, T, g)) for _ in range(REPS)])
            out[str(n)] = {'eps_ms': ms_e, 'eps_ms_per_1000': ms_e / n * 1000, 'vjp_ms': ms_v, 'vjp_ms_per_1000': ms_v / n * 1000}
    elif step == 'clear':
        eng.reserve_vjp(1)
        xs, gs, xl, gl = rand(8000, 1), rand(8000, 2, 1.0), rand(CLIP, 3), rand(CLIP, 4, 1.0)
        for name, short, long in (('eps', lambda: eng.wavenet_eps_len(xs, T), lambda: eng.wavenet_eps_len(xl, T)),
                                  ('vjp', lambda: eng.wavenet_eps_vjp_len(xs, T, gs), lambda: eng.wavenet_eps_vjp_len(xl, T, gl))):
            short(), long(), short()
            after_same, after_long = [], []
            for _ in range(REPS):
                after_same.append(timed(short))                                           # 8000 after 8000: nothing cleared
                long()
                after_long.append(timed(short))                                           # 8000 after 32000: the band is cleared first
                short()
            out[name] = {'after_8000_ms': median(after_same), 'after_32000_ms': median(after_long),
                         'clearing_ms': median(after_long) - median(after_same)}
    else:
        import torch.nn.functional as F
        from acoustic_system import AcousticSystem
        from audio_models.RCNN_KWS.model import KWSModel
        from diffusion_models.diffwave_ddpm import DiffWave, WaveNetHIP
        from diffusion_models.DiffWave_Unconditional.util import calc_diffusion_hyperparams
        from dmad_hip.transforms import KWSMelSpectrogramDB
        torch.manual_seed(7)
        net = KWSModel(in_size=32).cuda().eval().use_engine(eng)
        den = DiffWave(WaveNetHIP(eng, state_dict=sd, any_length=True), calc_diffusion_hyperparams(**synth.DIFFUSION_CONFIG), reverse_timestep=1)
        x, y, lr = rand(16000, 5).unsqueeze(1), torch.tensor([1], device='cuda'), 65 / 5 / 32768.0
        b0 = eng.device_bytes()
        eng.reserve_vjp(1)
        out['engine_vjp_workspace_bytes'] = eng.device_bytes() - b0
        for backend in ('hip', 'torch'):
            net.grad_backend = den.model.grad_backend = backend
            system = AcousticSystem(classifier=net, transform=KWSMelSpectrogramDB(eng, grad_backend=backend), defender=den, defense_type='wave')
            delta = torch.zeros_like(x, requires_grad=True)

            def iteration():
                loss = F.nll_loss(system(x + delta), y)
                loss.backward()
                delta.data = delta.data + lr * delta.grad.data.sign()
                delta.grad.zero_()
            iteration()
            torch.cuda.synchronize()
            torch.cuda.empty_cache()
            torch.cuda.reset_peak_memory_stats()
            base = torch.cuda.memory_allocated()
            iteration()
            torch.cuda.synchronize()
            grew = torch.cuda.max_memory_allocated() - base
            out[backend] = {'iteration_ms': median([timed(iteration) for _ in range(REPS)]), 'torch_peak_bytes': grew}
    eng.close()
    print(json.dumps(out), flush=True)


if __name__ == '__main__':
    if len(sys.argv) > 1:
        main(sys.argv[1])
    else:
        for name, limit in STEPS.items():                 # a step that fails, faults or runs out of time ends the run
            rc = subprocess.run(['timeout', '-k', '10', str(limit), sys.executable, os.path.abspath(__file__), name]).returncode
            if rc != 0:
                sys.exit('step %s ended with status %d: nothing more is started' % (name, rc))
