"""Cases of the any-length exact-fp32 WaveNet tests (tests/test_wavenet_len_cpu.py, tests/test_gpu_wavenet_len.py): geometries,
weights, inputs, lengths, and the float64 references, computed once per process and shared.

Geometries.  'small': 5 layers, dilation cycle 4 (largest dilation 8), clip_len 2048, max_batch 3.  'full': the reference's 36 x 12
(largest dilation 2048) at clip_len 4096, max_batch 2, so that d = 2048 exceeds half the clip.
Weights.  The synthetic state dicts with the final block's ReLU kept off its kink (the recipe of kink_free in
tests/test_gpu_wavenet_vjp.py, restated here because that file is a GPU test module): at a kink an fp32 pre-activation within ~1e-7 of
zero lands on the other side than float64's and ANY fp32 gradient differs from float64's by percents.  The CPU file checks, for every
case below, that the fp32 CPU oracle is within the tolerances of the float64 one, so that no kink decides a GPU test.
Lengths (small): 1 and 3 (fewer positions than taps), 7 (below the largest dilation), 127 / 128 / 129 (the edge of a GEMM column tile;
with B = 3 a tile straddles two clips), 1021 (prime, len % 4 == 1), 2047, 2048 (clip_len)."""
import functools

import numpy as np
import torch

from dmad_hip import synth

FP32_TOL = 2e-5         # eps against the float64 oracle, relative to max |eps|
VJP_TOL = 1e-4          # g_x against float64 autograd, relative to max |g_x|

GEOMETRY = {'small': dict(num_res_layers=5, dilation_cycle=4, clip_len=2048, max_batch=3, seed=77, t=12),
            'full': dict(num_res_layers=36, dilation_cycle=12, clip_len=4096, max_batch=2, seed=1234, t=40)}
SMALL_LENS = (1, 3, 7, 127, 128, 129, 1021, 2047, 2048)
EPS_CASES = tuple(('small', B, n) for B in (1, 3) for n in SMALL_LENS) + tuple(('full', 2, n) for n in (2047, 2049, 3001))
VJP_CASES = tuple(('small', B, n) for B in (1, 3) for n in SMALL_LENS) + (('full', 1, 2049),)
ALL_CASES = tuple(dict.fromkeys(EPS_CASES + VJP_CASES))


def case_id(case):
    return '%s-B%d-len%d' % case


def relmax(got, ref):
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    return np.abs(got - ref).max() / np.abs(ref).max()


def kink_free(sd):
    out = dict(sd)
    b = np.asarray(sd['final_conv.0.conv.bias'])
    out['final_conv.0.conv.bias'] = np.where(np.arange(b.shape[0]) % 2 == 0, 16.0, -16.0).astype(b.dtype)
    return out


def wavenet_config(geom):
    cfg = dict(synth.WAVENET_CONFIG)
    cfg.update(num_res_layers=GEOMETRY[geom]['num_res_layers'], dilation_cycle=GEOMETRY[geom]['dilation_cycle'])
    return cfg


@functools.lru_cache(maxsize=None)
def state_dict(geom):
    return kink_free(synth.wavenet_state_dict(GEOMETRY[geom]['seed'], wavenet_config(geom)))


def inputs(case):
    """(x [B, len], g_eps [B, len]) float32 on the CPU: the first len samples of synthetic clips at 0.8, a seeded normal co-vector"""
    geom, B, n = case
    x = torch.from_numpy(np.stack([synth.synthetic_clip(3 * i + 1)[0][:n] for i in range(B)])).float() * 0.8
    g = torch.randn((B, n), generator=torch.Generator().manual_seed(1000 * B + n))
    return x.contiguous(), g


@functools.lru_cache(maxsize=None)
def reference(case, dtype=torch.float64):
    """(eps [B, len], g_x [B, len]) numpy float64 of oracle.wavenet_forward and its autograd, computed in `dtype` on the CPU"""
    from oracle import dmad_oracle as orc
    geom, B, n = case
    G = GEOMETRY[geom]
    nl, cyc = G['num_res_layers'], G['dilation_cycle']
    w = {k: v.to(dtype) for k, v in orc.folded_weights(state_dict(geom), nl).items()}
    x, g = inputs(case)
    xx = x.to(dtype).unsqueeze(1).requires_grad_(True)
    eps = orc.wavenet_forward(w, xx, float(G['t']) * torch.ones((B, 1), dtype=dtype), nl, cyc)
    (gx,) = torch.autograd.grad(eps, xx, g.to(dtype).unsqueeze(1))
    return eps.detach()[:, 0].double().numpy(), gx[:, 0].double().numpy()
