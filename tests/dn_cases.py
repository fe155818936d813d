"""Shared by tests/test_densenet_cpu.py, tests/test_gpu_densenet.py and the recorders under tests/golden: the inputs and the references
of the DenseNet-BC-100-12 tests.

  * specs(B, seed): spectrograms in the dB range of the mel front-end (the helper of the other classifiers' VJP tests).
  * dn_walk: DenseNet-BC-100-12 (eval mode) in the dtype of its arguments, free (its own ReLU decisions, recorded) or PINNED to given
    decisions (pre * mask in place of relu).  A ReLU net evaluated in two arithmetic orders can take different branches at units within
    rounding of the kink; given the decisions the VJP is linear algebra, so the pinned walk checks every weight image, scale fold, tap
    flip, slice offset and routing of the engine without depending on which side of a near-tie fp32 landed.
    tests/test_densenet_cpu.py checks it against plain float64 autograd.
  * mask_conditions / logit_conditions: the non-vacuity conditions the stand-in weights must meet on TEST_INPUTS."""
import numpy as np
import torch
import torch.nn.functional as F

from dmad_hip.synth import DN_BLOCKS as BLOCKS, DN_GROWTH as GROWTH, DN_LAYERS as LAYERS, DN_SEED  # noqa: F401  (the geometry is stated once, with the stand-in)

N_MAPS = 99
TEST_INPUTS = ((2, 1), (3, 12), (5, 2), (7, 3), (2, 6))      # (B, seed) of the spectrogram batches the GPU tests use


def specs(B, seed=0):
    g = torch.Generator().manual_seed(seed)
    return (torch.rand(B, 1, 32, 32, generator=g) * 60.0 - 70.0).float()      # the dB range of the mel front-end


def relmax(got, ref):
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    return np.abs(got - ref).max() / np.abs(ref).max()


def _sd(sd, dtype):
    return {k: torch.from_numpy(np.asarray(v)).to(dtype) if np.asarray(v).dtype.kind == 'f' else torch.from_numpy(np.asarray(v))
            for k, v in sd.items()}


def sd64(sd):
    return _sd(sd, torch.float64)


def sd32(sd):
    return _sd(sd, torch.float32)


def dn_walk(sd, x, decisions=None):
    """DenseNet-BC-100-12 (eval mode) on x [B,1,32,32] in the dtype of sd / x.  decisions None: the free forward (relu), which records its
    decisions; decisions = masks: the pinned forward — masks[k] (bool, the shape of pre-activation k, k = 0..98) multiplies pre-activation
    k.  The 99 slots in forward order: o and h of a block's 16 layers, then the transition's (behind dense3: the final) map.  Returns
    (logits, rec) with rec['maps'] the post-ReLU maps (NCHW), rec['pre'] the pre-activations, rec['masks'], rec['taps'] the outputs of
    dense1 and trans2 (the fixture's taps)."""
    rec = dict(maps=[], pre=[], masks=[], taps={})

    def act(pre):
        k = len(rec['maps'])
        m = (pre > 0) if decisions is None else decisions[k]
        rec['pre'].append(pre)
        rec['masks'].append(m)
        h = pre * m.to(pre.dtype)
        rec['maps'].append(h)
        return h

    def bn(h, p):
        return F.batch_norm(h, sd[p + 'running_mean'], sd[p + 'running_var'], sd[p + 'weight'], sd[p + 'bias'], False, 0.0, 1e-5)

    x = F.conv2d(x, sd['conv1.weight'], None, 1, 1)
    for blk in range(3):
        for i in range(LAYERS):
            p = 'dense%d.%d.' % (blk + 1, i)
            o = act(bn(x, p + 'bn1.'))
            h = act(bn(F.conv2d(o, sd[p + 'conv1.weight']), p + 'bn2.'))
            x = torch.cat((x, F.conv2d(h, sd[p + 'conv2.weight'], None, 1, 1)), 1)
        if blk == 0:
            rec['taps']['dense1'] = x
        if blk < 2:
            p = 'trans%d.' % (blk + 1)
            x = F.avg_pool2d(F.conv2d(act(bn(x, p + 'bn1.')), sd[p + 'conv1.weight']), 2)
            if blk == 1:
                rec['taps']['trans2'] = x
    f = act(bn(x, 'bn.'))
    return F.linear(f.mean((2, 3)), sd['fc.weight'], sd['fc.bias']), rec


def pinned_vjp(sd, x, g, decisions):
    """(g_spec [B,32,32], rec) of the pinned walk, in the dtype of sd, for the cotangent g [B,num_classes]"""
    dtype = sd['conv1.weight'].dtype
    x = x.detach().to(dtype).requires_grad_(True)
    logits, rec = dn_walk(sd, x, decisions)
    (gx,) = torch.autograd.grad((logits * g.to(dtype)).sum(), x)
    return gx[:, 0], rec


def tap_slices(taps):
    """the subsampled taps tests/golden/densenet_bc_100_12.npz stores: dense1's output [B,216,32,32] and trans2's [B,150,8,8]"""
    return taps['dense1'][:, ::18, ::5, ::7], taps['trans2'][:, ::15]


def mask_conditions(masks):
    """the per-map conditions on one batch's 99 ReLU masks: alive on between 5 % and 95 % of the units, and two rows differ"""
    assert len(masks) == N_MAPS
    for j, m in enumerate(masks):
        frac = float(m.double().mean())
        assert 0.05 < frac < 0.95, ('alive fraction of map %d' % j, frac)
        assert not torch.equal(m[0], m[1]), ('rows 0 and 1 share the mask of map %d' % j)


def logit_conditions(logits):
    """logits: the rows of every batch of TEST_INPUTS: at least 3 classes predicted, top-2 margins of order one"""
    lg = np.asarray(logits, np.float64)
    srt = np.sort(lg, 1)
    margin = np.median(srt[:, -1] - srt[:, -2])
    classes = len(set(lg.argmax(1).tolist()))
    assert classes >= 3, classes
    assert 0.1 < margin < 10.0, margin
    return classes, margin
