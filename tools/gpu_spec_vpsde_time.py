#!/usr/bin/env python3
"""Time the reverse VP-SDE spectrogram purifier (diffusion_models/improved_diffusion_sde.py; dmad_spec_vpsde_purify / _vjp) on a DMAD_FP32
engine with the synthetic UNet of the reference geometry, for B in {8, 20, 64} (20: the adaptive-attack driver's default batch) and t in
{2, 5, 25}: the inference chain (path 0), the 'hip' forward (exact-fp32 tier, trajectory kept) and the full-gradient backward, in ms per
spectrogram per Euler step; against the UNet's forward (dmad_unet_eps, tier 0) and its VJP (dmad_unet_eps_vjp) at the same B, which gives
the share of the chain's time outside the UNet (diffusion draw, step kernel, the affine epilogue).  Memory: the UNet VJP reservation,
and over a 'hip' forward + backward through RevImprovedDiffusion at t = 5 the growth of torch's allocator and of the engine.  HIP events
after a warm-up, medians of REPS rounds.  Prints one JSON line (profiles/r09_spec_vpsde.md)."""
import json
import os
import sys
import types

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, 'diffusion-model-for-audio-defense_amd')
sys.path[:0] = [ROOT, PKG]
from diffusion_models import improved_diffusion_sde as SDE  # noqa: E402
from diffusion_models.improved_diffusion_ddpm import create_improved_diffusion  # noqa: E402
from dmad_hip import engine as E, synth  # noqa: E402

BATCHES = [int(b) for b in os.environ.get('BATCHES', '8,20,64').split(',')]
TS = [int(t) for t in os.environ.get('TS', '2,5,25').split(',')]
REPS = int(os.environ.get('REPS', 3))

sd = synth.unet_state_dict(5252)
eng = E.Engine(max_batch=max(BATCHES), precision=E.FP32, with_classifier=False, with_wavenet=False)
create_improved_diffusion(None, state_dict=sd, engine=eng)
b0 = eng.device_bytes()
eng.reserve_unet_vjp(max(BATCHES))
res = {'reps': REPS, 'engine_bytes_before_reservation': b0, 'unet_vjp_reservation_bytes': eng.device_bytes() - b0, 'B': {}}


def timed(fn, reps=REPS):
    fn()                                   # warm-up
    out = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b))
    return sorted(out)[len(out) // 2]


def peak(fn):
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    fn()
    torch.cuda.synchronize()
    return torch.cuda.max_memory_allocated() - base


for B in BATCHES:
    gen = torch.Generator('cuda').manual_seed(B)
    x = torch.rand(B, 32, 32, device='cuda', generator=gen) * 1.6 - 0.8
    g = torch.randn(B, 32, 32, device='cuda', generator=gen)
    # the UNet alone at this B (step 25: the scale-shift rows are cached per step, any step costs the same)
    eps_fwd = timed(lambda: eng.unet_eps(x, 25, tier=0))
    eps_vjp = timed(lambda: eng.unet_eps_vjp(x, 25, g))
    rb = {'unet_eps_ms_per_spec': eps_fwd / B, 'unet_eps_vjp_ms_per_spec': eps_vjp / B, 't': {}}
    for t in TS:
        sch = SDE.spec_vpsde_schedule(t)
        S = sch.steps
        a = (sch.c_a, sch.c_b, sch.k, sch.h, sch.hb, sch.q, sch.gs)
        keep = {}

        def fwd_traj():
            keep['traj'] = eng.spec_vpsde_purify(x, *a, seed=1, path=1, want_traj=True)[1]

        def bwd():
            eng.spec_vpsde_purify_vjp(keep['traj'], sch.c_a, sch.k, sch.h, sch.hb, sch.q, g)
        f_inf = timed(lambda: eng.spec_vpsde_purify(x, *a, seed=1))
        f_traj = timed(fwd_traj)
        b_ms = timed(bwd)
        rb['t'][t] = {
            'steps': S,
            'ms_per_spec_per_step': {'forward': f_inf / B / S, 'forward_hip': f_traj / B / S, 'backward_hip': b_ms / B / S},
            # the share of the chain's time outside S UNet evaluations (forward) / S UNet VJPs (backward)
            'forward_overhead_vs_S_eps': f_inf / (S * eps_fwd) - 1, 'forward_hip_overhead_vs_S_eps': f_traj / (S * eps_fwd) - 1,
            'backward_overhead_vs_S_vjp': b_ms / (S * eps_vjp) - 1,
        }
    res['B'][B] = rb

# memory of the 'hip' mode through the module at t = 5, B = 8
args = types.SimpleNamespace(ddpm_path=None, t=5, score_type='guided_diffusion', sample_step=1, rand_t=False, t_delta=0, use_bm=False)
den = SDE.RevImprovedDiffusion(args, state_dict=sd, engine=eng, score_grad='hip')
s = (torch.rand(8, 1, 32, 32, device='cuda') * 1.6 - 0.8) * 40.0 - 40.0


def module_step():
    sr = s.clone().requires_grad_(True)
    torch.autograd.grad(den(sr).sum(), sr)


module_step()
bytes_before = eng.device_bytes()
res['hip_t5_B8_torch_alloc_growth'] = peak(module_step)
res['hip_t5_B8_trajectory_bytes'] = (5 + 1) * 8 * 1024 * 4
res['hip_t5_B8_engine_bytes_growth'] = eng.device_bytes() - bytes_before
print(json.dumps(res))
eng.close()
