"""Shared by tests/test_vgg_vjp_cpu.py and tests/test_gpu_vgg_vjp.py: the inputs and the float64 references of the VGG19_bn VJP tests.

  * specs(B, seed): spectrograms in the dB range of the mel front-end (the helper of the ResNeXt29 VJP test).
  * pool_case / pool_relu_bwd_ref: integer-valued maps with every tie the pool + ReLU backward has a rule for, and its float64 reference.
  * vgg_walk: VGG19_bn in float64, free (its own ReLU / max-pool decisions, recorded with their margins) or PINNED to given decisions
    (pre * mask in place of relu, a gather at the given arg-max in place of max_pool2d).  A ReLU / max-pool net evaluated in two
    arithmetic orders can take different branches at units within rounding of a kink; given the decisions the VJP is linear algebra, so
    the pinned walk checks every weight image, scale fold, tap flip and routing of the engine without depending on which side of a
    near-tie fp32 landed.  tests/test_vgg_vjp_cpu.py checks these references against plain float64 autograd."""
import numpy as np
import torch
import torch.nn.functional as F

VGG19_CFG = [64, 64, 'M', 128, 128, 'M', 256, 256, 256, 256, 'M', 512, 512, 512, 512, 'M', 512, 512, 512, 512, 'M']
VJP_TOL = 1e-4          # relative to max |g|: the tolerance of every VJP test of the project
FP32_TOL = 2e-5         # the project's bound for the fp32 tier against a reference, relative to the map's max
VGG_SEED = 4321


def specs(B, seed=0):
    g = torch.Generator().manual_seed(seed)
    return (torch.rand(B, 1, 32, 32, generator=g) * 60.0 - 70.0).float()      # the dB range of the mel front-end


def relmax(got, ref):
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    return np.abs(got - ref).max() / np.abs(ref).max()


def sd64(sd):
    return {k: torch.from_numpy(np.asarray(v)).double() if np.asarray(v).dtype.kind == 'f' else torch.from_numpy(np.asarray(v))
            for k, v in sd.items()}


# ---- the pool + ReLU backward -------------------------------------------------------------------------------------------------------
def windows(h):
    """[..., H, W] -> [..., H/2, W/2, 4]: every 2x2 window in scan order (top-left, top-right, bottom-left, bottom-right)"""
    return torch.stack([h[..., 0::2, 0::2], h[..., 0::2, 1::2], h[..., 1::2, 0::2], h[..., 1::2, 1::2]], -1)


def first_max(w):
    """index of the first maximum along the last axis (torch's max_pool2d keeps the earlier entry on a tie)"""
    top = w.max(-1, keepdim=True).values
    return ((w == top).cumsum(-1) == 0).sum(-1)


def unwindows(w):
    """inverse of windows()"""
    out = w.new_zeros(w.shape[:-3] + (2 * w.shape[-3], 2 * w.shape[-2]))
    out[..., 0::2, 0::2], out[..., 0::2, 1::2], out[..., 1::2, 0::2], out[..., 1::2, 1::2] = w.unbind(-1)
    return out


def pool_relu_bwd_ref(g, y):
    """float64 reference of launch_vgg_pool_relu_bwd on NHWC maps: g [B,H/2,H/2,C], y [B,H,H,C] -> gpre [B,H,H,C]."""
    w = windows(y.double().permute(0, 3, 1, 2))
    a = first_max(w)
    on = (w.max(-1).values > 0).double() * g.double().permute(0, 3, 1, 2)
    return unwindows(F.one_hot(a, 4).double() * on.unsqueeze(-1)).permute(0, 2, 3, 1).contiguous()


def pool_case(B, H, C, seed):
    """y [B,H,H,C] of small integers in [-3, 3] and g [B,H/2,H/2,C]: random windows (ties are frequent at seven values), and in the
    leading channels of every pooled pixel the decisive ones: a positive tie in every pair of window positions (the other two entries
    lower), ties of three and four, a single maximum at each position, an all-zero window, an all-negative window with a tie, and a
    window whose maximum is zero above negatives."""
    gen = torch.Generator().manual_seed(seed)
    y = torch.randint(-3, 4, (B, H, H, C), generator=gen).float()
    g = torch.randint(1, 8, (B, H // 2, H // 2, C), generator=gen).float() * 0.25 - 1.0        # no zero: a routed gradient is visible
    g[g == 0] = 2.0
    special = []
    for p in range(4):
        for q in range(p + 1, 4):
            lo = [1.0, -3.0]
            special.append([2.0 if i in (p, q) else lo.pop() for i in range(4)])
    special += [[3.0, 3.0, 3.0, 1.0], [0.0, 2.0, 2.0, 2.0], [1.0, 1.0, 1.0, 1.0]]
    special += [[3.0 if i == p else 1.0 for i in range(4)] for p in range(4)]
    special += [[0.0, 0.0, 0.0, 0.0], [-1.0, -3.0, -1.0, -2.0], [-2.0, 0.0, -1.0, 0.0]]
    yw = windows(y.permute(0, 3, 1, 2))                      # [B,C,Hp,Hp,4]
    for c, w in enumerate(special):
        yw[:, c] = torch.tensor(w)
    return unwindows(yw).permute(0, 2, 3, 1).contiguous(), g


# ---- the whole network ----------------------------------------------------------------------------------------------------------
def vgg_walk(sd, x, decisions=None):
    """VGG19_bn (eval mode) on x [B,1,32,32] in the dtype of sd / x.  decisions None: the free forward — relu and first-maximum
    pooling — which records its decisions and their margins.  decisions = (masks, args): the pinned forward — masks[k] (bool, the
    shape of conv / FC output k, k = 0..17) multiplies pre-activation k, args[j] (long [B,C,H/2,H/2], 0..3) picks pool j's entry.
    Returns (logits, rec) with rec['maps'] the 18 post-ReLU maps (NCHW; FC: [B,4096]), rec['pre'] the 18 pre-activations, rec['masks'],
    rec['args'], rec['gaps'] (per pool the top-2 gap of every window)."""
    rec = dict(maps=[], pre=[], masks=[], args=[], gaps=[])

    def act(pre):
        k = len(rec['maps'])
        m = (pre > 0) if decisions is None else decisions[0][k]
        rec['pre'].append(pre)
        rec['masks'].append(m)
        h = pre * m.to(pre.dtype)
        rec['maps'].append(h)
        return h

    idx = 0
    for v in VGG19_CFG:
        if v == 'M':
            w = windows(x)
            a = first_max(w) if decisions is None else decisions[1][len(rec['args'])]
            top2 = w.sort(-1, descending=True).values
            rec['args'].append(a)
            rec['gaps'].append(top2[..., 0] - top2[..., 1])
            x = w.gather(-1, a.unsqueeze(-1)).squeeze(-1)
            idx += 1
            continue
        x = F.conv2d(x, sd['features.%d.weight' % idx], sd['features.%d.bias' % idx], padding=1)
        b = 'features.%d.' % (idx + 1)
        x = act(F.batch_norm(x, sd[b + 'running_mean'], sd[b + 'running_var'], sd[b + 'weight'], sd[b + 'bias'], False, 0.0, 1e-5))
        idx += 3
    x = x.reshape(x.shape[0], -1)
    x = act(F.linear(x, sd['classifier.0.weight'], sd['classifier.0.bias']))
    x = act(F.linear(x, sd['classifier.3.weight'], sd['classifier.3.bias']))
    return F.linear(x, sd['classifier.6.weight'], sd['classifier.6.bias']), rec


def tape_decisions(tape):
    """The decisions an engine's tape records: tape = the 18 post-ReLU maps (conv maps NCHW).  ReLU masks y > 0; a pool's arg-max is the
    first maximum of its input map, the rule of the backward kernel."""
    masks = [t > 0 for t in tape]
    args, k = [], -1
    for v in VGG19_CFG:
        if v == 'M':
            args.append(first_max(windows(tape[k])))
        else:
            k += 1
    return masks, args


def pinned_vjp(sd, x, g, decisions):
    """(g_spec [B,32,32], rec) of the pinned float64 walk for the cotangent g [B,num_classes]"""
    x = x.detach().double().requires_grad_(True)
    logits, rec = vgg_walk(sd, x, decisions)
    (gx,) = torch.autograd.grad((logits * g.double()).sum(), x)
    return gx[:, 0], rec


def pool_input_index():
    """index (0..15) of the conv map each of the five pools reads"""
    out, k = [], -1
    for v in VGG19_CFG:
        if v == 'M':
            out.append(k)
        else:
            k += 1
    return out
