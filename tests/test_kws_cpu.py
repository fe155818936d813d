"""The attention-CRNN keyword spotter, the part that needs no GPU: the mirror audio_models/RCNN_KWS/model.py and the step-by-step float64
walk of tests/kws_cases.py against the fixture recorded from the reference (tests/golden/kws_vanilla.npz, made by
tests/golden/make_golden_kws.py), the structural zeros of the input gradient, the B = 1 shape, the host semantics of the module, and
the C ABI of the three exports and its binding."""
import copy
import ctypes
import os
import pickle
import re
import subprocess

import numpy as np
import pytest
import torch

import kws_cases as kc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, 'diffusion-model-for-audio-defense_amd')
LIB = os.path.join(PKG, 'libdmad_hip.so')
NEW_EXPORTS = {'dmad_kws_logits': 7, 'dmad_kws_vjp': 8, 'dmad_kws_tape': 7}       # name -> arguments


def mirror(dtype=torch.float32):
    from audio_models.RCNN_KWS.model import KWSModel
    net = KWSModel(in_size=32)
    net.load_state_dict(kc.state_dict())
    return net.to(dtype).eval()


def test_fixture_is_not_vacuous():
    fx = kc.fixture()
    assert tuple(fx['cases']) == kc.CASES and len(fx['keys']) == 24
    classes = set()
    for T in kc.CASES:
        lp = fx['logp64_%d' % T]
        assert fx['spec_%d' % T].shape == (3, 1, 32, T) and lp.shape == (3, 4) and lp.dtype == np.float64
        assert np.exp(lp).max(axis=1).min() < 0.9            # an undecided row
        assert np.abs(fx['gspec64_%d' % T]).max() >= 1e-2
        assert 0 < fx['err_logp_%d' % T] < 1e-4 and 0 < fx['err_g_%d' % T] < 1e-5       # fp32 round-off, not a bug in the recording
        classes.update(lp.argmax(axis=1).tolist())
    assert len(classes) >= 2


def test_mirror_state_dict_is_the_references():
    fx = kc.fixture()
    sd = mirror().state_dict()
    assert list(sd.keys()) == [str(k) for k in fx['keys']]
    for k, v in sd.items():
        assert tuple(v.shape) == fx['w.' + k].shape, k
    assert sum(v.numel() for v in sd.values()) == sum(fx['w.' + str(k)].size for k in fx['keys'])


@pytest.mark.parametrize('T', kc.CASES)
def test_mirror_float64_equals_the_recorded_reference(T):
    fx = kc.fixture()
    net = mirror(torch.float64)
    x = torch.from_numpy(fx['spec_%d' % T].copy()).double().requires_grad_(True)
    logp = net(x, torch.zeros(4, 3, 64, dtype=torch.float64))       # like the reference, the mirror's own `hidden` is float32
    (logp * torch.from_numpy(fx['g_%d' % T].copy()).double()).sum().backward()
    assert (logp.detach().numpy() - fx['logp64_%d' % T]).__abs__().max() < 1e-12
    assert np.abs(x.grad.numpy() - fx['gspec64_%d' % T]).max() < 1e-12


@pytest.mark.parametrize('T', kc.CASES)
def test_walk_equals_the_recorded_reference_and_autograd_stage_by_stage(T):
    fx = kc.fixture()
    spec, g = torch.from_numpy(fx['spec_%d' % T].copy()), torch.from_numpy(fx['g_%d' % T].copy())
    out = kc.kws_walk(kc.state_dict(), spec, g)
    assert (out['logp'].numpy() - fx['logp64_%d' % T]).__abs__().max() < 1e-12
    assert np.abs(out['g_spec'].numpy() - fx['gspec64_%d' % T][:, 0]).max() < 1e-12
    # the stages against the mirror's own layers (nn.GRU and all) in float64
    net, S = mirror(torch.float64), kc.steps(T)
    with torch.no_grad():
        x = spec.double()[:, 0]
        x0 = net.CRNN_model.sepconv(x).permute(2, 0, 1)
        states = []
        inp = x0
        gru = net.CRNN_model.gru
        for l in range(2):                                   # layer by layer: a one-layer GRU with the layer's parameters
            one = torch.nn.GRU(inp.shape[2], 64, num_layers=1, bidirectional=True).double()
            for sfx in ('', '_reverse'):
                for k in ('weight_ih', 'weight_hh', 'bias_ih', 'bias_hh'):
                    getattr(one, '%s_l0%s' % (k, sfx)).copy_(getattr(gru, '%s_l%d%s' % (k, l, sfx)))
            inp, _ = one(inp, torch.zeros(2, 3, 64, dtype=torch.float64))
            states.append(inp)
        e = torch.cat([net.attn_layer(el) for el in states[1]], dim=1)
    assert tuple(out['x0'].shape) == (3, S, 64) and tuple(out['h1'].shape) == (3, S, 128) and tuple(out['e'].shape) == (3, S)
    assert (out['x0'] - x0.transpose(0, 1)).abs().max().item() < 1e-12
    assert (out['h0'] - states[0].transpose(0, 1)).abs().max().item() < 1e-12
    assert (out['h1'] - states[1].transpose(0, 1)).abs().max().item() < 1e-12
    assert (out['e'] - e).abs().max().item() < 1e-12


@pytest.mark.parametrize('T', kc.CASES)
def test_walk_backward_is_exactly_zero_outside_the_frames_that_are_read(T):
    fx = kc.fixture()
    g_spec = kc.kws_walk(kc.state_dict(), torch.from_numpy(fx['spec_%d' % T].copy()), torch.from_numpy(fx['g_%d' % T].copy()))['g_spec'].numpy()
    m = kc.support(T)
    assert m.sum() == 5 * kc.steps(T)
    assert (g_spec[:, :, ~m] == 0.0).all() and (fx['gspec64_%d' % T][:, 0][:, :, ~m] == 0.0).all()
    assert (np.abs(g_spec[:, :, m]).max(axis=(0, 1)) > 0).all()           # and every frame that is read gets a gradient


def test_steps():
    assert [kc.steps(T) for T in (5, 20, 21, 37, 81, 501, 644, 645)] == [1, 1, 2, 3, 5, 32, 40, 41]
    from dmad_hip import engine as E
    assert [E.kws_steps(T) for T in (4, 5, 20, 21, 81, 501, 644)] == [0, 1, 1, 2, 5, 32, 40] and E.KWS_MAX_T == 644


def test_batch_of_one_keeps_its_row():
    fx = kc.fixture()
    net = mirror()
    x = torch.from_numpy(fx['spec_81'][:1].copy())
    with torch.no_grad():
        one = net(x)
    assert tuple(one.shape) == (1, 4) and tuple(net(x[:, 0]).shape) == (1, 4)
    assert np.abs(one.numpy() - fx['logp32_81'][:1]).max() < 1e-5
    assert tuple(kc.kws_walk(kc.state_dict(), x)['logp'].shape) == (1, 4)


def test_module_host_semantics(monkeypatch):
    """grad_backend, use_engine's binding call, __getstate__, and which calls take the torch layers -- with a recording engine"""
    from audio_models.RCNN_KWS.model import KWSModel, is_kws
    from dmad_hip import engine as E
    net = mirror()
    assert is_kws(net) and not is_kws(torch.nn.Linear(2, 2)) and not hasattr(net, 'bind_engine')
    assert net.grad_backend == 'auto'
    with pytest.raises(ValueError, match='grad_backend'):
        net.grad_backend = 'cuda'
    net.grad_backend = 'hip'
    assert KWSModel().in_size == 40 and KWSModel().CRNN_model.sepconv[1].groups == 2        # the reference's defaults

    class Recorder:
        calls = []

        def kws_logits(self, x):
            self.calls.append(tuple(x.shape))
            return torch.zeros(x.shape[0], 4)

    bound = []
    monkeypatch.setattr(E, 'bind_kws', lambda sd, ks, st, eng: bound.append((sorted(sd), ks, st, eng)) or Recorder())
    assert net.use_engine() is net and bound[0][1:] == ((20, 5), (8, 2), None) and len(bound[0][0]) == 24
    assert 'engine' not in net.state_dict() and 'engine' not in pickle.loads(pickle.dumps(net)).__dict__
    assert 'engine' not in copy.deepcopy(net).__dict__ and copy.deepcopy(net).grad_backend == 'hip'
    x = torch.from_numpy(kc.fixture()['spec_21'].copy())
    with torch.no_grad():
        ref = mirror()(x)
        assert torch.equal(net(x), ref) and Recorder.calls == []            # a CPU input never reaches the engine
        assert torch.equal(net(x, torch.zeros(4, 3, 64)), ref)
    net.train()
    assert net(x).shape == (3, 4) and Recorder.calls == []


def test_acoustic_system_does_not_take_kws_for_the_spectrogram_classifier():
    """a KWSModel's `engine` attribute must not send AcousticSystem.query() down the one-call chain of the 32 x 32 classifiers, even when
    that engine holds one and the transform looks like the engine's mel front-end"""
    import types
    from acoustic_system import AcousticSystem
    net = mirror()
    net.__dict__['engine'] = types.SimpleNamespace(has_classifier=True, has_m5=False, has_kws=True)
    mel = types.SimpleNamespace(transforms=[types.SimpleNamespace(_dmad_stage='mel_power'), types.SimpleNamespace(_dmad_stage='power_to_db')])
    assert AcousticSystem(net, mel, None)._engine_chain(True) == (None, 0)
    assert AcousticSystem(net, None, None)._engine_chain(True) == (None, 0)
    spec = torch.from_numpy(kc.fixture()['spec_21'].copy())
    system = AcousticSystem(net, lambda x: spec.repeat(x.shape[0] // 3, 1, 1, 1), None)
    logits, dec = system.query(torch.zeros(3, 1, 8), 2)              # loops over forward(): the module's torch layers on the CPU
    assert tuple(logits.shape) == (2, 3, 4) and np.abs(logits[1].numpy() - kc.fixture()['logp32_21']).max() < 1e-5


def test_load_checkpoint_passes_map_location(tmp_path, monkeypatch):
    from audio_models.RCNN_KWS import model as M
    path = str(tmp_path / 'kws.pth')
    torch.save(kc.state_dict(), path)
    seen = []
    real = torch.load
    monkeypatch.setattr(torch, 'load', lambda f, *a, **k: seen.append(k.get('map_location')) or real(f, *a, **k))
    net = M.load_checkpoint(path)
    assert seen == ['cpu'] and not net.training and net.in_size == 32
    assert all(torch.equal(v, kc.state_dict()[k]) for k, v in net.state_dict().items())


@pytest.fixture(scope='module')
def built_lib():
    if not os.path.exists(LIB):
        subprocess.run(['make', '-C', os.path.join(PKG, 'csrc'), '-j4'], check=True)
    return ctypes.CDLL(LIB)


def test_kws_exports(built_lib):
    hdr = re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', 'dmad.h')).read(), flags=re.S)
    from dmad_hip import _lib
    for name, nargs in NEW_EXPORTS.items():
        m = re.search(r'\bint\s+%s\s*\(([^)]*)\)\s*;' % name, hdr)
        assert m and len(m.group(1).split(',')) == nargs, name
        assert hasattr(built_lib, name), name
        assert name in _lib.EXPORTS and len(_lib._SIGNATURES[name][1]) == nargs, name
    P, i32 = ctypes.c_void_p, ctypes.c_int32
    assert _lib._SIGNATURES['dmad_kws_vjp'] == (ctypes.c_int, [P, P, i32, i32, P, P, P, P])
    assert _lib._SIGNATURES['dmad_kws_tape'] == (ctypes.c_int, [P, P, i32, i32, i32, P, P])
