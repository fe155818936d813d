#!/usr/bin/env python3
"""BUILD-CONTAINER-ONLY generator of tests/golden/densenet_bc_100_12.npz: logits (and two intermediate taps) of the imported reference's
`models.densenet.DenseNet(depth=100, growthRate=12, compressionRate=2, num_classes=10, in_channels=1)` — the zoo's `densenet_bc_100_12` —
loaded with the build's seeded synthetic weights (dmad_hip/synth.py), on the mel spectrograms of tests/golden/classifiers.npz, plus the
list of the reference's state-dict keys with their shapes.  The taps: dense1's output, and trans2's output (its conv reads a stream
whose width 300 is no multiple of 16).

Usage:  python tests/golden/make_golden_densenet.py
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden as mg  # noqa: E402  (shims + path setup only)


def main():
    torch.set_num_threads(8)
    mg.install_shims()
    from dmad_hip import synth
    from models.densenet import DenseNet         # the reference's audio_models/ConvNets_SpeechCommands/models (make_golden.REF)
    assert sys.modules['models.densenet'].__file__.startswith(mg.REF + os.sep)
    net = DenseNet(depth=100, growthRate=12, compressionRate=2, num_classes=10, in_channels=1)
    net.load_state_dict(mg.to_torch_sd(synth.densenet_bc_100_12_state_dict(synth.DN_SEED)))
    net.eval()
    with np.load(os.path.join(HERE, 'classifiers.npz')) as z:
        spec = torch.from_numpy(z['spec_in'])
    taps = {}
    hooks = [net.dense1.register_forward_hook(lambda m, i, o: taps.__setitem__('dense1', o.detach()[:, ::18, ::5, ::7].numpy().copy())),
             net.trans2.register_forward_hook(lambda m, i, o: taps.__setitem__('trans2', o.detach()[:, ::15].numpy().copy()))]
    with torch.no_grad():
        logits = net(spec)
    for h in hooks:
        h.remove()
    print(logits)
    state = net.state_dict()
    keys = np.array(list(state.keys()))
    shapes = np.array([','.join(str(d) for d in v.shape) for v in state.values()])
    np.savez_compressed(os.path.join(HERE, 'densenet_bc_100_12.npz'), spec_in=spec.numpy(), logits=logits.numpy(), dense1=taps['dense1'],
                        trans2=taps['trans2'], seed=np.array(synth.DN_SEED), keys=keys, shapes=shapes)


if __name__ == '__main__':
    main()
