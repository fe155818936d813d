#!/usr/bin/env python3
"""Time the WaveNet vector-Jacobian product (dmad_wavenet_eps_vjp, forward-save included) against the torch restatement's
forward + backward (dmad_hip/autograd.py) and the exact-fp32 forward alone, at B clips (default 8), step t = 40, in one process:
HIP events after warm-up, REPS interleaved rounds, medians.  Peak memory: growth of torch's allocator over a forward + backward
for both branches, plus the engine's VJP workspace (dmad_device_bytes before / after dmad_reserve_vjp, outside torch's allocator).
Prints one JSON line (profiles/r06_wavenet_vjp.md)."""
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, 'diffusion-model-for-audio-defense_amd')]
from dmad_hip import autograd as AG, engine as E, synth  # noqa: E402

B, T, REPS = int(os.environ.get('B', 8)), 40, int(os.environ.get('REPS', 5))
NL, L = 36, 16000
PEAK_TF = 157.3                       # fp32 matrix peak of the MI355X (dense, spec)
# FLOP per clip from shapes: forward (dil 3 x 512 x 256, res + skip 2 x 256 x 256 per layer, f0) and the backward's recompute of H,
# res / skip transposed (K = 512 over two taps; the last layer K = 256), dilated transposed (3 x 256 x 512)
F_FWD = 2 * L * (NL * (3 * 512 * 256 + 2 * 256 * 256) + 256 * 256)
F_BWD = 2 * L * (NL * 3 * 512 * 256 + (2 * NL - 1) * 256 * 256 + NL * 3 * 256 * 512 + 256 * 256)

sd = synth.wavenet_state_dict(1234)
eng = E.Engine(max_batch=B, precision=E.FP32, with_classifier=False)
eng.load_wavenet(sd)
b0 = eng.device_bytes()
eng.reserve_vjp(B)
ws = eng.device_bytes() - b0
fw = AG.FoldedWaveNet(E.fold_wavenet_state_dict(sd, NL), NL, 12)
x = torch.randn(B, 1, L, device='cuda', generator=torch.Generator('cuda').manual_seed(1)) * 0.3
g = torch.randn(B, 1, L, device='cuda', generator=torch.Generator('cuda').manual_seed(2))


def hip_vjp():
    return eng.wavenet_eps_vjp(x, T, g)


def torch_fb():
    xg = x.clone().requires_grad_(True)
    eps = AG.wavenet_eps(fw, xg, T)
    return torch.autograd.grad(eps, xg, g)[0]


def fwd():
    return eng.wavenet_eps(x, T)


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def peak(fn):
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    fn()
    torch.cuda.synchronize()
    return torch.cuda.max_memory_allocated() - base


for fn in (hip_vjp, torch_fb, fwd):   # warm-up
    fn()
mem = {'hip_torch_alloc': peak(hip_vjp), 'torch': peak(torch_fb)}
ms = {'hip_vjp': [], 'torch_fwd_bwd': [], 'fp32_fwd': []}
for _ in range(REPS):
    ms['hip_vjp'].append(timed(hip_vjp))
    ms['torch_fwd_bwd'].append(timed(torch_fb))
    ms['fp32_fwd'].append(timed(fwd))
med = {k: sorted(v)[len(v) // 2] for k, v in ms.items()}
gx_h, gx_t = hip_vjp(), torch_fb()[:, 0]
out = {
    'B': B, 't': T, 'reps': REPS, 'ms_median': med, 'ms_min': {k: min(v) for k, v in ms.items()},
    'ms_per_clip': {k: v / B for k, v in med.items()},
    'tflop_per_clip': {'vjp': (F_FWD + F_BWD) / 1e12, 'fwd': F_FWD / 1e12},
    'vjp_tflops': B * (F_FWD + F_BWD) / med['hip_vjp'] / 1e9, 'fwd_tflops': B * F_FWD / med['fp32_fwd'] / 1e9,
    'vjp_share_of_fp32_peak': B * (F_FWD + F_BWD) / med['hip_vjp'] / 1e9 / PEAK_TF,
    'fwd_share_of_fp32_peak': B * F_FWD / med['fp32_fwd'] / 1e9 / PEAK_TF,
    'peak_bytes': {'torch_branch': mem['torch'], 'hip_branch_torch_alloc': mem['hip_torch_alloc'], 'hip_vjp_workspace': ws},
    'relmax_hip_vs_torch': float((gx_h - gx_t).abs().max() / gx_t.abs().max()),
}
print(json.dumps(out))
eng.close()
