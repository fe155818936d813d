#!/usr/bin/env python3
"""BUILD-CONTAINER-ONLY generator of tests/golden/kws_vanilla.npz: the imported reference's `audio_models/RCNN_KWS/model.py::KWSModel`
(in_size = 32) with its shipped state dict `vanilla-best-acc-kws-attn_rcnn-n_mels=32.pth`, run on the CPU in float64 and in float32.

The file holds the 24 tensors of the state dict (`w.<key>`, and `keys` in the state dict's order) and, for T in CASES,
  spec_<T>      float32 [3,1,32,T] = randn * 15 - 30 (a dB-like range), g_<T> float32 [3,4] = randn, from one seeded generator
  logp64_<T>    float64 [3,4], gspec64_<T> float64 [3,1,32,T]: the module in float64 and d(sum(logp * g)) / d spec
  logp32_<T>    float32, gspec32_<T> float32: the same from the float32 module
  err_logp_<T>  max |logp32 - logp64|;  err_g_<T>  max |gspec32 - gspec64| / max |gspec64|: the float32 module's own error, the
                yardstick the engine is measured with (4 x, tests/test_gpu_kws.py)
The reference builds `hidden` with a float32 torch.zeros, so its float64 run is given a float64 `hidden` explicitly.

Usage:  python tests/golden/make_golden_kws.py
"""
import importlib.util
import os

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REF = '/root/reference'
CKPT = os.path.join(REF, 'audio_models', 'RCNN_KWS', 'checkpoints', 'vanilla-best-acc-kws-attn_rcnn-n_mels=32.pth')
CASES = (5, 20, 21, 37, 81, 501)
SEED, B = 2207, 3


def reference_module():
    """the reference's model.py by its file path: the name `audio_models` belongs to this project's package on sys.path"""
    spec = importlib.util.spec_from_file_location('reference_rcnn_kws_model', os.path.join(REF, 'audio_models', 'RCNN_KWS', 'model.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def run(net, spec, g, dtype):
    x = spec.detach().clone().to(dtype).requires_grad_(True)
    hidden = torch.zeros(net.gru_num_layers * 2, x.shape[0], net.hidden_size, dtype=dtype)
    logp = net(x, hidden)
    assert tuple(logp.shape) == (x.shape[0], 4)
    (logp * g.to(dtype)).sum().backward()
    return logp.detach(), x.grad.detach()


def main():
    torch.set_num_threads(8)
    ref = reference_module()
    state = torch.load(CKPT, map_location='cpu')
    assert len(state) == 24
    net32 = ref.KWSModel(in_size=32)
    net32.load_state_dict(state)
    net32.eval()
    net64 = ref.KWSModel(in_size=32)
    net64.load_state_dict(state)
    net64.double().eval()
    out = {'keys': np.array(list(state.keys())), 'cases': np.array(CASES), 'seed': np.array(SEED)}
    for k, v in state.items():
        assert v.dtype == torch.float32
        out['w.' + k] = v.numpy()
    gen = torch.Generator().manual_seed(SEED)
    classes = set()
    for T in CASES:
        spec = torch.randn(B, 1, 32, T, generator=gen) * 15 - 30
        g = torch.randn(B, 4, generator=gen)
        lp64, gs64 = run(net64, spec, g, torch.float64)
        lp32, gs32 = run(net32, spec, g, torch.float32)
        assert lp64.dtype == torch.float64 and gs64.dtype == torch.float64 and lp32.dtype == torch.float32
        err_lp = (lp32.double() - lp64).abs().max().item()
        err_g = ((gs32.double() - gs64).abs().max() / gs64.abs().max()).item()
        # the fixture must be able to fail: an undecided row, a gradient that is not vanishing, more than one class overall
        pmax = lp64.exp().max(dim=1).values
        assert pmax.min().item() < 0.9, (T, pmax)
        assert gs64.abs().max().item() >= 1e-2, (T, gs64.abs().max())
        classes.update(lp64.argmax(dim=1).tolist())
        print('T = %3d  classes %s  p_max %s  max|g| %.3g  fp32 error: logp %.3g  gradient %.3g of its maximum'
              % (T, lp64.argmax(dim=1).tolist(), ['%.2f' % p for p in pmax.tolist()], gs64.abs().max().item(), err_lp, err_g))
        out.update({'spec_%d' % T: spec.numpy(), 'g_%d' % T: g.numpy(), 'logp64_%d' % T: lp64.numpy(), 'gspec64_%d' % T: gs64.numpy(),
                    'logp32_%d' % T: lp32.numpy(), 'gspec32_%d' % T: gs32.numpy(), 'err_logp_%d' % T: np.array(err_lp),
                    'err_g_%d' % T: np.array(err_g)})
    assert len(classes) >= 2, classes
    path = os.path.join(HERE, 'kws_vanilla.npz')
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), 'bytes')
    assert os.path.getsize(path) < (1 << 20)


if __name__ == '__main__':
    main()
