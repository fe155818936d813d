#!/usr/bin/env python3
"""Time the reverse VP-SDE purifier (diffusion_models/diffwave_sde.py; dmad_vpsde_purify / dmad_vpsde_purify_vjp) at B clips (default 8)
on a DMAD_FP32 engine with synthetic weights of the reference geometry, for t in {2, 5, 30}: the inference chain, the chain with its
trajectory kept ('hip' forward) and the full-gradient backward, in ms per clip; against S x the eps-network forward and S x its VJP
alone at the same B, which gives the share of the per-step work outside the eps-network (step kernel, diffusion draw, the affine
epilogue).  Memory: growth of torch's allocator over a 'hip' forward + backward at t = 5, and the engine's bytes.  The 'torch' mode
(the eps-network's torch restatement composed with the same draws) at t = 2 for comparison.  HIP events after warm-up, medians of
REPS rounds.  Prints one JSON line (profiles/r07_vpsde.md)."""
import json
import os
import sys
import types

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, 'diffusion-model-for-audio-defense_amd')
sys.path[:0] = [ROOT, PKG]
from diffusion_models import diffwave_sde as SDE  # noqa: E402
from dmad_hip import engine as E, synth  # noqa: E402

B, REPS = int(os.environ.get('B', 8)), int(os.environ.get('REPS', 3))
L = 16000

sd = synth.wavenet_state_dict(1234)
eng = E.Engine(max_batch=B, precision=E.FP32, with_classifier=False)
eng.load_wavenet(sd)
b0 = eng.device_bytes()
eng.reserve_vjp(B)
reservation = eng.device_bytes() - b0
x = torch.randn(B, 1, L, device='cuda', generator=torch.Generator('cuda').manual_seed(1)) * 0.3
g = torch.randn(B, L, device='cuda', generator=torch.Generator('cuda').manual_seed(2))


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


res = {'B': B, 'reps': REPS, 'engine_bytes_before_reservation': b0, 'vjp_reservation_bytes': reservation, 't': {}}
# the eps-network alone at this B, for the per-step reference (step index 10: any step costs the same)
eps_fwd = timed(lambda: eng.wavenet_eps(x, 10))
eps_vjp = timed(lambda: eng.wavenet_eps_vjp(x, 10, g))
res['eps_forward_ms'], res['eps_vjp_ms'] = eps_fwd, eps_vjp
for t in (2, 5, 30):
    sch = SDE.vpsde_schedule(t)
    S = sch.steps
    a = (sch.c_a, sch.c_b, sch.k, sch.h, sch.hb, sch.q, sch.gs)
    keep = {}

    def fwd_traj():
        keep['traj'] = eng.vpsde_purify(x, *a, seed=1, path=1, want_traj=True)[1]

    def bwd():
        eng.vpsde_purify_vjp(keep['traj'], sch.c_a, sch.k, sch.h, sch.hb, sch.q, g)
    f_inf = timed(lambda: eng.vpsde_purify(x, *a, seed=1))
    f_traj = timed(fwd_traj)
    b_ms = timed(bwd)
    res['t'][t] = {
        'steps': S, 'k': sch.k.tolist(),
        'ms_per_clip': {'forward': f_inf / B, 'forward_traj': f_traj / B, 'backward': b_ms / B, 'forward_plus_backward': (f_traj + b_ms) / B},
        'backward_per_step_ms_per_clip': b_ms / B / S,
        # the share of the chain's time outside S eps evaluations (forward) / S eps VJPs (backward)
        'forward_overhead_vs_S_eps': f_inf / (S * eps_fwd) - 1, 'forward_traj_overhead_vs_S_eps': f_traj / (S * eps_fwd) - 1,
        'backward_overhead_vs_S_vjp': b_ms / (S * eps_vjp) - 1,
        'trajectory_bytes': (S + 1) * B * L * 4,
    }

# allocator growth of the 'hip' mode over a forward + backward through the module at t = 5 (B clips)
args = types.SimpleNamespace(ddpm_path=None, ddpm_config=os.path.join(PKG, 'configs', 'config.json'), t=5, score_type='guided_diffusion',
                             sample_step=1, rand_t=False, t_delta=0, use_bm=False)
den = SDE.RevDiffWave(args, state_dict=sd, engine=eng, score_grad='hip')


def module_step():
    xg = x.clone().requires_grad_(True)
    torch.autograd.grad(den(xg).sum(), xg)


bytes_before = eng.device_bytes()
res['hip_t5_torch_alloc_growth'] = peak(module_step)
res['hip_t5_engine_bytes_growth'] = eng.device_bytes() - bytes_before

# the 'torch' mode at t = 2: the same gradient through the eps-network's torch restatement
args.t = 2
den_t = SDE.RevDiffWave(args, state_dict=sd, engine=eng, score_grad='torch')
den_h = SDE.RevDiffWave(args, state_dict=sd, engine=eng, score_grad='hip')


def step_of(d):
    def run():
        d._draws = 0
        xg = x.clone().requires_grad_(True)
        return torch.autograd.grad((den_out := d(xg)).mul(g.view_as(den_out)).sum(), xg)[0]
    return run


res['t2_modes'] = {
    'torch_ms_per_clip': timed(step_of(den_t), 1) / B, 'hip_ms_per_clip': timed(step_of(den_h)) / B,
    'torch_alloc_growth': peak(step_of(den_t)), 'hip_alloc_growth': peak(step_of(den_h)),
}
gh, gt = step_of(den_h)(), step_of(den_t)()
lin = SDE.vpsde_schedule(2).linear_gain() * g.view_as(gh)
res['t2_modes']['eps_part_rel_diff_hip_vs_torch'] = float((gh - gt).norm() / (gh - lin).norm())
res['t2_modes']['eps_part_share_of_gradient'] = float((gh - lin).norm() / gh.norm())
print(json.dumps(res))
eng.close()
