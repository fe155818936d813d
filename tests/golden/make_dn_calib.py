#!/usr/bin/env python3
"""BUILD-CONTAINER tool: calibration data that keep the synthetic DenseNet-BC-100-12 stand-in (dmad_hip/synth.py, seed 10012) from being
degenerate, modelled on tests/golden/make_wrn_calib.py.

A randomly initialised 100-layer DenseNet with arbitrary BatchNorm statistics predicts ONE class with margins of tens of logit units and
leaves whole ReLU maps dead or fully alive: a VJP test on such a stand-in would pass with a mask read from the wrong row, layer or
pixel.  ONE BatchNorm calibration pass over spectrograms in the mel front-end's dB range gives every BatchNorm the statistics of what it
actually sees; the linear head is then centred on the mean pooled feature and scaled to a logit spread of 1.5.

The result is DATA (99 BatchNorms' running statistics + the adjusted head), committed beside this script under tests/golden/ so that
every machine loads bit-identical parameters.  Everything runs on the CPU.  The conditions the tests rely on (tests/dn_cases.py) are
checked here, on the committed parameters, and again by tests/test_densenet_cpu.py.

    python tests/golden/make_dn_calib.py
"""
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
PKG = os.path.join(ROOT, 'diffusion-model-for-audio-defense_amd')
sys.path[:0] = [ROOT, PKG, os.path.join(ROOT, 'tests')]
from dmad_hip import synth  # noqa: E402
import dn_cases as D  # noqa: E402

DATA = os.path.dirname(os.path.abspath(__file__))
TARGET_LOGIT_STD = 1.5
CALIB = ((24, 1000), (24, 1001))          # (rows, seed) of the calibration spectrograms: none of the tests' seeds


def dn_calibrate(sd, x):
    """One pass of the network in which every BatchNorm takes the statistics of this batch (and keeps them as its running statistics).
    Returns (new statistics, pooled features [n, 342])."""
    T = D.sd32(sd)
    out = {}

    def bn(h, p):
        m, v = h.mean((0, 2, 3)), h.var((0, 2, 3), unbiased=False)
        out[p + '.running_mean'], out[p + '.running_var'] = m.numpy().astype(np.float32), v.numpy().astype(np.float32)
        return F.batch_norm(h, m, v, T[p + '.weight'], T[p + '.bias'], False, 0.0, 1e-5)

    x = F.conv2d(x, T['conv1.weight'], None, 1, 1)
    for blk in range(3):
        for i in range(D.LAYERS):
            p = 'dense%d.%d' % (blk + 1, i)
            h = F.relu(bn(F.conv2d(F.relu(bn(x, p + '.bn1')), T[p + '.conv1.weight']), p + '.bn2'))
            x = torch.cat((x, F.conv2d(h, T[p + '.conv2.weight'], None, 1, 1)), 1)
        if blk < 2:
            p = 'trans%d' % (blk + 1)
            x = F.avg_pool2d(F.conv2d(F.relu(bn(x, p + '.bn1')), T[p + '.conv1.weight']), 2)
    return out, F.relu(bn(x, 'bn')).mean((2, 3))


def check_conditions(sd):
    """the stand-in's conditions (tests/dn_cases.py) on the tests' inputs, in fp32 on the CPU"""
    net, rows = D.sd32(sd), []
    for B, seed in D.TEST_INPUTS:
        with torch.no_grad():
            logits, rec = D.dn_walk(net, D.specs(B, seed))
        D.mask_conditions(rec['masks'])
        alive = [float(m.float().mean()) for m in rec['masks']]
        print('  B = %d seed %d: alive fractions %.2f .. %.2f, predictions %s' % (B, seed, min(alive), max(alive), logits.argmax(1).tolist()))
        rows.append(logits)
    classes, margin = D.logit_conditions(torch.cat(rows).numpy())
    print('  %d classes predicted, median top-2 margin %.3f' % (classes, margin))


def main():
    torch.set_num_threads(8)
    sd = synth.densenet_bc_100_12_state_dict(synth.DN_SEED, calibrated=False)
    x = torch.cat([D.specs(B, seed) for B, seed in CALIB])
    with torch.no_grad():
        stats, feat = dn_calibrate(sd, x)
        Wt, b = torch.from_numpy(sd['fc.weight']), torch.from_numpy(sd['fc.bias'])
        mu = feat.mean(0)
        z = F.linear(feat - mu, Wt)
        s = TARGET_LOGIT_STD / float(z.std())
        W2 = (Wt * s).float()
        b2 = (b - F.linear(mu[None], W2)[0]).float()
        print('head centred on the mean feature and scaled by %.2f: logit std %.3f' % (s, float(F.linear(feat, W2, b2).std())))
    stats['fc.weight'] = W2.numpy().astype(np.float32)
    stats['fc.bias'] = b2.numpy().astype(np.float32)
    path = os.path.join(DATA, 'densenet_bc_100_12_calib_seed%d.npz' % synth.DN_SEED)
    np.savez_compressed(path, **stats)
    print('wrote %d arrays, %d floats -> %s (%d bytes)' % (len(stats), sum(v.size for v in stats.values()), path, os.path.getsize(path)))
    check_conditions(synth.densenet_bc_100_12_state_dict(synth.DN_SEED))


if __name__ == '__main__':
    main()
