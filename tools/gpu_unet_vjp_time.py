#!/usr/bin/env python3
"""Time the UNet vector-Jacobian product (dmad_unet_eps_vjp, the forward with its tape included) against the exact-fp32 forward alone,
at B in {8, 64, 256} spectrograms, step t = 25: HIP events after warm-up, REPS rounds, medians.  FLOP from synth.unet_layout (the
GEMM work of the forward; the backward's transposed convs are the same shapes minus the input conv, plus the attention backward as
this kernel computes it).  Also: the VJP workspace (dmad_device_bytes), the torch allocator's growth over a SpecPurifier forward +
backward, and that chain's time at t* = 3 and t* = 25 (B = 8).  Prints one JSON line (profiles/r08_unet_vjp.md)."""
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, 'diffusion-model-for-audio-defense_amd')]
from diffusion_models.improved_diffusion_ddpm import SpecPurifier, create_improved_diffusion  # noqa: E402
from dmad_hip import engine as E, synth  # noqa: E402

BS, T, REPS = (8, 64, 256), 25, int(os.environ.get('REPS', 5))
PEAK_TF = 157.3                       # fp32 matrix peak of the MI355X (dense, spec)


def flops():
    _, inp, mid, outp = synth.unet_layout()
    fwd = bwd = att_f = att_b = 0
    H = 32
    for p, kind, ci, co in [m for b in inp for m in b] + list(mid) + [m for b in outp for m in b]:
        px = H * H
        if kind == 'conv_in':
            fwd += 2 * 9 * co * px
            bwd += 2 * 9 * co * px
        elif kind == 'res':
            f = 2 * 9 * px * (ci * co + co * co) + (2 * px * ci * co if ci != co else 0)
            fwd += f; bwd += f
        elif kind == 'attn':
            f = 2 * px * (3 * ci * ci + ci * ci)
            fwd += f; bwd += f
            att_f += 2 * 2 * px * px * ci                     # S = Q K^T, O = P V over the 4 heads of 64
            att_b += 2 * 8 * px * px * ci                     # the kernel's 8 T x T x 64 products (S three times, dP three, dV, dK, dQ)
        elif kind == 'down':
            fwd += 2 * 9 * ci * co * px // 4
            bwd += 2 * 9 * ci * co * px                       # on the zero-dilated map (3/4 of it multiplies zeros)
        elif kind == 'up':
            H *= 2
            fwd += 2 * 9 * ci * co * H * H
            bwd += 2 * 9 * ci * co * H * H
        if kind == 'down':
            H //= 2
    fwd += 2 * 9 * 128 * 1024
    bwd += 2 * 9 * 128 * 1024
    return fwd, att_f, bwd, att_b


def timed(fn, reps=REPS):
    fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        out.append(a.elapsed_time(b))
    return sorted(out)[len(out) // 2]


def main():
    F_FWD, F_ATT, F_BWD, F_ATTB = flops()
    eng = E.Engine(max_batch=max(BS), precision=E.FP32, with_classifier=False, with_wavenet=False)
    pur = create_improved_diffusion(None, reverse_timestep=3, state_dict=synth.unet_state_dict(5252), engine=eng)
    res = {'gflop_fwd': (F_FWD + F_ATT) / 1e9, 'gflop_vjp_bwd': (F_BWD + F_ATTB) / 1e9, 'gflop_attn_bwd': F_ATTB / 1e9, 'per_B': {}}
    g = torch.Generator(device='cuda').manual_seed(0)
    for B in BS:
        b0 = eng.device_bytes()
        eng.reserve_unet_vjp(B)
        ws = eng.device_bytes() - b0
        x = torch.rand(B, 32, 32, device='cuda', generator=g) * 2 - 1
        ge = torch.randn(B, 32, 32, device='cuda', generator=g)
        fwd = timed(lambda: eng.unet_eps(x, T, tier=0))
        vjp = timed(lambda: eng.unet_eps_vjp(x, T, ge))
        bwd = vjp - fwd
        res['per_B'][B] = {'fwd_ms_per_spec': fwd / B, 'vjp_ms_per_spec': vjp / B, 'bwd_only_ms_per_spec': bwd / B,
                           'fwd_peak_share': (F_FWD + F_ATT) * B / (fwd * 1e-3) / (PEAK_TF * 1e12),
                           'bwd_peak_share': (F_BWD + F_ATTB) * B / (bwd * 1e-3) / (PEAK_TF * 1e12),
                           'workspace_grow_mb': ws / 2 ** 20}
    res['engine_bytes_mb'] = eng.device_bytes() / 2 ** 20
    for ts in (3, 25):
        pur.reverse_timestep = ts
        den = SpecPurifier(pur, seed=1)
        s = (torch.rand(8, 1, 32, 32, device='cuda', generator=g) * 80 - 80).requires_grad_(True)

        def chain():
            s.grad = None
            den(s).sum().backward()
        torch.cuda.synchronize()
        base = torch.cuda.memory_allocated()
        torch.cuda.reset_peak_memory_stats()
        ms = timed(chain, 3)
        res['spec_purifier_t%d' % ts] = {'fwd_bwd_ms_B8': ms, 'alloc_growth_mb': (torch.cuda.max_memory_allocated() - base) / 2 ** 20}
    print(json.dumps(res))
    eng.close()


if __name__ == '__main__':
    main()
