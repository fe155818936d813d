"""Shared by tests/test_wrn_cpu.py, tests/test_gpu_wrn.py and the recorders under tests/golden: the inputs and the float64 references of
the WideResNet-28-10 tests.

  * specs(B, seed): spectrograms in the dB range of the mel front-end (the helper of the VGG19_bn and ResNeXt29 VJP tests).
  * wrn_walk: WideResNet-28-10 (eval mode) in the dtype of its arguments, free (its own ReLU decisions, recorded) or PINNED to given
    decisions (pre * mask in place of relu).  A ReLU net evaluated in two arithmetic orders can take different branches at units within
    rounding of the kink, and two such flips out of 4.6 million move this network's free input gradient by 3.5e-3 of its maximum; given
    the decisions the VJP is linear algebra, so the pinned walk checks every weight image, scale fold, tap flip, shortcut and routing of the
    engine without depending on which side of a near-tie fp32 landed.  tests/test_wrn_cpu.py checks it against plain float64 autograd.
  * conditions(...): the non-vacuity conditions the stand-in weights must meet on TEST_INPUTS."""
import numpy as np
import torch
import torch.nn.functional as F

from dmad_hip.synth import WRN_BLOCKS as BLOCKS, WRN_SEED, WRN_WIDTHS as WIDTHS  # noqa: F401  (the geometry is stated once, with the stand-in)

VJP_TOL = 1e-4          # relative to max |g|: the tolerance of every VJP test of the project
FP32_TOL = 2e-5         # the project's bound for the fp32 tier against a reference, relative to the map's max
TEST_INPUTS = ((2, 1), (3, 12), (5, 2), (7, 3), (2, 6))      # (B, seed) of the spectrogram batches the GPU tests use


def specs(B, seed=0):
    g = torch.Generator().manual_seed(seed)
    return (torch.rand(B, 1, 32, 32, generator=g) * 60.0 - 70.0).float()      # the dB range of the mel front-end


def relmax(got, ref):
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    return np.abs(got - ref).max() / np.abs(ref).max()


def sd64(sd):
    return {k: torch.from_numpy(np.asarray(v)).double() if np.asarray(v).dtype.kind == 'f' else torch.from_numpy(np.asarray(v))
            for k, v in sd.items()}


def sd32(sd):
    return {k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()}


def block_prefix(i):
    return 'block%d.layer.%d.' % (i // 4 + 1, i % 4)


def wrn_walk(sd, x, decisions=None):
    """WideResNet-28-10 (eval mode) on x [B,1,32,32] in the dtype of sd / x.  decisions None: the free forward (relu), which records its
    decisions; decisions = masks: the pinned forward — masks[k] (bool, the shape of pre-activation k, k = 0..24) multiplies pre-activation
    k.  The 25 slots in forward order: o and h of blocks 0..11, then the final map.  Returns (logits, rec) with rec['maps'] the post-ReLU
    maps (NCHW), rec['pre'] the pre-activations, rec['masks'], rec['taps'] the outputs of block1 and block3 (the fixture's taps)."""
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
    for i, (cin, cout, stride) in enumerate(BLOCKS):
        p = block_prefix(i)
        o = act(bn(x, p + 'bn1.'))
        h = act(bn(F.conv2d(o, sd[p + 'conv1.weight'], None, stride, 1), p + 'bn2.'))
        short = x if cin == cout else F.conv2d(o, sd[p + 'convShortcut.weight'], None, stride)      # the 1x1 reads the ACTIVATED input
        x = short + F.conv2d(h, sd[p + 'conv2.weight'], None, 1, 1)
        if i % 4 == 3:
            rec['taps']['block%d' % (i // 4 + 1)] = x
    f = act(bn(x, 'bn1.'))
    return F.linear(f.mean((2, 3)), sd['fc.weight'], sd['fc.bias']), rec


def pinned_vjp(sd, x, g, decisions):
    """(g_spec [B,32,32], rec) of the pinned float64 walk for the cotangent g [B,num_classes]"""
    x = x.detach().double().requires_grad_(True)
    logits, rec = wrn_walk(sd, x, decisions)
    (gx,) = torch.autograd.grad((logits * g.double()).sum(), x)
    return gx[:, 0], rec


def tap_slices(taps):
    """the subsampled taps tests/golden/wideresnet28_10.npz stores: block1's output [B,160,32,32] and block3's [B,640,8,8]"""
    return taps['block1'][:, ::16, ::5, ::7], taps['block3'][:, ::64]


def mask_conditions(masks):
    """the per-map conditions on one batch's 25 ReLU masks: alive on between 5 % and 95 % of the units, and two rows differ"""
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
