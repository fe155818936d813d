#!/usr/bin/env python3
"""BUILD-CONTAINER-ONLY generator of tests/golden/wideresnet28_10.npz: logits (and two intermediate taps) of the imported reference's
`models.wideresnet.WideResNet(depth=28, widen_factor=10, dropRate=0, num_classes=10, in_channels=1)` — the zoo's `wideresnet28_10` —
loaded with the build's seeded synthetic weights (dmad_hip/synth.py), on the mel spectrograms of tests/golden/classifiers.npz, plus the
list of the reference's state-dict keys with their shapes.

Usage:  python tests/golden/make_golden_wrn.py
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
    from models.wideresnet import WideResNet         # the reference's audio_models/ConvNets_SpeechCommands/models (make_golden.REF)
    assert sys.modules['models.wideresnet'].__file__.startswith(mg.REF + os.sep)
    net = WideResNet(depth=28, widen_factor=10, dropRate=0, num_classes=10, in_channels=1)
    net.load_state_dict(mg.to_torch_sd(synth.wideresnet28_10_state_dict(synth.WRN_SEED)))
    net.eval()
    with np.load(os.path.join(HERE, 'classifiers.npz')) as z:
        spec = torch.from_numpy(z['spec_in'])
    taps = {}
    hooks = [net.block1.register_forward_hook(lambda m, i, o: taps.__setitem__('block1', o.detach()[:, ::16, ::5, ::7].numpy().copy())),
             net.block3.register_forward_hook(lambda m, i, o: taps.__setitem__('block3', o.detach()[:, ::64].numpy().copy()))]
    with torch.no_grad():
        logits = net(spec)
    for h in hooks:
        h.remove()
    print(logits)
    state = net.state_dict()
    keys = np.array(list(state.keys()))
    shapes = np.array([','.join(str(d) for d in v.shape) for v in state.values()])
    np.savez_compressed(os.path.join(HERE, 'wideresnet28_10.npz'), spec_in=spec.numpy(), logits=logits.numpy(), block1=taps['block1'],
                        block3=taps['block3'], seed=np.array(synth.WRN_SEED), keys=keys, shapes=shapes)


if __name__ == '__main__':
    main()
