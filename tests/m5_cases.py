"""Shared by tests/test_m5_cpu.py and tests/test_gpu_m5.py: the inputs and the float64 references of the M5 tests.

  * real_sd() / synth_sd(): the trained kernel_size = 160 checkpoint (tests/golden/m5_k160_state.npz, 10 classes) and the synthetic
    k = 80 geometry, synth.m5_state_dict(7, 80, 35).
  * clips(n): synth.synthetic_clip(0..n-1) as [n,1,16000]: the full clip length, at which all four pool remainders occur
    (991 = 4 * 247 + 3, 245 = 4 * 61 + 1, 59 = 4 * 14 + 3).
  * m5_walk: M5 (eval mode) in the dtype of sd / x, free (ReLU and first-maximum pooling; it records each pooled unit's decision
    arg | on << 2 and the pre-pool maps) or PINNED to given decisions (pooled = on * pre[4 p + arg] in place of relu and max_pool1d).
    A ReLU / max-pool net evaluated in two arithmetic orders can take different branches at units within rounding of a kink; given the
    decisions the VJP is linear algebra, so the pinned walk checks every weight image, scale, route and gather of the engine without
    depending on which side of a near-tie fp32 landed.  tests/test_m5_cpu.py checks the walk against oracle.m5_forward and plain
    float64 autograd.
  * pool_route_ref / pool_case: the pool + ReLU routing rule on integer maps with every tie among 4 positions."""
import os

import numpy as np
import torch
import torch.nn.functional as F

VJP_TOL = 1e-4          # relative to max |g| per clip: the tolerance of every VJP test of the project
FP32_TOL = 2e-5         # the project's bound for the fp32 tier against a reference, relative to the map's max
L = 16000
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')


def real_sd():
    with np.load(os.path.join(GOLDEN, 'm5_k160_state.npz')) as z:
        return {k: z[k] for k in z.files}


def synth_sd():
    from dmad_hip import synth
    return dict(synth.m5_state_dict(7, 80, 35))


def golden_clips():
    with np.load(os.path.join(GOLDEN, 'classifiers.npz')) as z:
        return torch.from_numpy(z['wave_in']).float(), torch.from_numpy(z['m5_logp']).float()


def clips(n, first=0):
    from dmad_hip import synth
    return torch.from_numpy(np.stack([synth.synthetic_clip(i) for i in range(first, first + n)])).float()       # [n,1,L]


def sd_t(sd, dtype=torch.float64):
    return {k: (torch.from_numpy(np.asarray(v)).to(dtype) if np.asarray(v).dtype.kind == 'f' else torch.from_numpy(np.asarray(v)))
            for k, v in sd.items()}


def module(sd):
    """the torch module (audio_models/M5/M5Net.py) holding sd, in eval mode"""
    from audio_models.M5.M5Net import M5
    m = M5(n_input=1, first_kernel_size=np.asarray(sd['conv1.weight']).shape[2], n_output=np.asarray(sd['fc1.weight']).shape[0])
    m.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()})
    return m.eval()


def first_max(w):
    """index of the first maximum along the last axis (torch's max_pool1d keeps the earlier entry on a tie)"""
    top = w.max(-1, keepdim=True).values
    return ((w == top).cumsum(-1) == 0).sum(-1)


def m5_walk(sd, x, decisions=None, stride=16):
    """M5 (eval mode) on x [B,1,L] in the dtype of sd / x.  decisions None: the free forward, which records its decisions; decisions =
    [dec1..dec4] (uint8 [B,C,T], arg | on << 2): the pinned forward.  Returns (logp, rec): rec['pre'] the four post-BatchNorm pre-ReLU
    maps [B,C,Tc], rec['pooled'] the four pooled post-ReLU maps [B,C,T], rec['dec'] the decisions."""
    rec = dict(pre=[], pooled=[], dec=[])
    for i in (1, 2, 3, 4):
        x = F.conv1d(x, sd['conv%d.weight' % i], sd['conv%d.bias' % i], stride=stride if i == 1 else 1)
        b = 'bn%d.' % i
        pre = F.batch_norm(x, sd[b + 'running_mean'], sd[b + 'running_var'], sd[b + 'weight'], sd[b + 'bias'], False, 0.0, 1e-5)
        T = pre.shape[-1] // 4
        w = pre[..., :4 * T].reshape(pre.shape[0], pre.shape[1], T, 4)           # the pool drops the remainder frames
        if decisions is None:
            r = torch.relu(w)
            a = first_max(r)
            on = r.max(-1).values > 0
        else:
            d = decisions[i - 1].to(torch.int64)
            a, on = d & 3, (d >> 2) > 0
        x = w.gather(-1, a.unsqueeze(-1)).squeeze(-1) * on.to(pre.dtype)
        rec['pre'].append(pre)
        rec['pooled'].append(x)
        rec['dec'].append((a + 4 * on.long()).to(torch.uint8))
    x = x.mean(-1)
    return F.log_softmax(F.linear(x, sd['fc1.weight'], sd['fc1.bias']), dim=1), rec


def pinned_vjp(sd64, x, g, decisions):
    """g_x [B,L] of the pinned float64 walk for the cotangent g [B,n_output]"""
    x = x.detach().double().requires_grad_(True)
    logp, rec = m5_walk(sd64, x, decisions)
    (gx,) = torch.autograd.grad((logp * g.double()).sum(), x)
    return gx[:, 0], rec


def kink_distance(rec64, layer, dec):
    """For every pooled unit of block `layer` (0..3) whose decision `dec` differs from the free float64 walk rec64: how far the float64
    pre-pool map is from the kink that separates the two decisions -- |relu(pre)[arg] - relu(pre)[arg64]| where the arg-max differs,
    |max pre| where only the sign of the maximum does.  Returns (number of differing units, the largest distance, max |pre|)."""
    pre = rec64['pre'][layer]
    T = pre.shape[-1] // 4
    w = pre[..., :4 * T].reshape(pre.shape[0], pre.shape[1], T, 4)
    r = torch.relu(w)
    d, d64 = dec.to(torch.int64).cpu(), rec64['dec'][layer].to(torch.int64)
    diff = d != d64
    ga = (r.gather(-1, (d & 3).unsqueeze(-1)) - r.gather(-1, (d64 & 3).unsqueeze(-1))).squeeze(-1).abs()
    gs = torch.where((d >> 2) != (d64 >> 2), w.max(-1).values.abs(), torch.zeros_like(ga))
    dist = torch.maximum(ga, gs)[diff]
    return int(diff.sum()), float(dist.max()) if dist.numel() else 0.0, float(pre.abs().max())


# ---- the pool + ReLU routing ----------------------------------------------------------------------------------------------------
def pool_route_ref(pre, g):
    """float64 reference of the routing rule: pre [C,Tc] (the BatchNorm output), g [C,T] -> the gradient at pre [C,Tc]: each window's g
    goes to the first maximum of relu(pre) and only where that maximum is > 0; remainder frames get 0."""
    pre, g = pre.double(), g.double()
    T = pre.shape[-1] // 4
    w = torch.relu(pre[:, :4 * T].reshape(pre.shape[0], T, 4))
    a = first_max(w)
    on = (w.max(-1).values > 0).double() * g
    out = torch.zeros_like(pre)
    out[:, :4 * T] = (F.one_hot(a, 4).double() * on.unsqueeze(-1)).reshape(pre.shape[0], 4 * T)
    return out


def pool_case(seed=0, C=8, extra=3):
    """pre [C,4 * n + extra] of small integers and g [C,n]: every positive tie among 2, 3 and 4 of the 4 positions, a single maximum at
    each position, an all-zero window, an all-negative window with a tie, a zero maximum above negatives, then random windows (ties are
    frequent at seven values); `extra` remainder frames that the pool drops (set high: they must get no gradient)."""
    special = []
    for p in range(4):
        for q in range(p + 1, 4):
            lo = [1.0, -3.0]
            special.append([2.0 if i in (p, q) else lo.pop() for i in range(4)])
    special += [[3.0, 3.0, 3.0, 1.0], [0.0, 2.0, 2.0, 2.0], [2.0, 1.0, 2.0, 2.0], [1.0, 1.0, 1.0, 1.0]]
    special += [[3.0 if i == p else 1.0 for i in range(4)] for p in range(4)]
    special += [[0.0, 0.0, 0.0, 0.0], [-1.0, -3.0, -1.0, -2.0], [-2.0, 0.0, -1.0, 0.0]]
    gen = torch.Generator().manual_seed(seed)
    n = len(special) + 8
    w = torch.randint(-3, 4, (C, n, 4), generator=gen).float()
    w[:, :len(special)] = torch.tensor(special)
    pre = torch.cat([w.reshape(C, 4 * n), torch.full((C, extra), 5.0)], 1)
    g = torch.randint(1, 8, (C, n), generator=gen).float() * 0.25 + 0.25          # no zero: a routed gradient is visible
    return pre, g
