"""The fused randomized-smoothing baseline (dmad_rs_smooth_votes / dmad_m5_rs_smooth_votes), the part that needs no GPU: the two exports
through the header, the library and the ctypes table, their loud refusal without an engine, and which route RobustCertificate takes for
which (classifier, transform) pair, decided on stand-in objects."""
import ctypes
import os
import re
import subprocess

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, 'diffusion-model-for-audio-defense_amd')
LIB = os.path.join(PKG, 'libdmad_hip.so')
EXPORTS = ('dmad_rs_smooth_votes', 'dmad_m5_rs_smooth_votes')


@pytest.fixture(scope='module')
def built_lib():
    if not os.path.exists(LIB):
        subprocess.run(['make', '-C', os.path.join(PKG, 'csrc'), '-j4'], check=True)
    return ctypes.CDLL(LIB)


def test_header_declares_both_exports_and_cites_the_reference():
    hdr = open(os.path.join(ROOT, 'include', 'dmad.h')).read()
    for name in EXPORTS:
        m = re.search(r'/\*((?:(?!\*/).)*)\*/\s*int %s\(dmad_engine\* e, const float\* clip, float sigma, int64_t n,' % name, hdr, flags=re.S)
        assert m, name
        assert 'certified_robust.py:34-67' in m.group(1) and 'denoiser is None' in m.group(1), name


def test_abi_names_both_exports(built_lib):
    from dmad_hip import _lib
    P, f, i64, i32, u64 = ctypes.c_void_p, ctypes.c_float, ctypes.c_int64, ctypes.c_int32, ctypes.c_uint64
    assert _lib._SIGNATURES['dmad_rs_smooth_votes'] == (ctypes.c_int, [P, P, f, i64, i32, u64, u64, P, P, P, P])
    assert _lib._SIGNATURES['dmad_m5_rs_smooth_votes'] == (ctypes.c_int, [P, P, f, i64, u64, u64, P, P, P, P])
    for name in EXPORTS:
        assert name in _lib.EXPORTS and hasattr(built_lib, name), name


def test_both_fail_loudly_without_an_engine():
    """No GPU, hence no engine handle: the calls return DMAD_ERR_INVALID with a message instead of touching anything."""
    from dmad_hip import _lib
    lib = _lib.load()
    buf = (ctypes.c_float * 4)()
    cnt = (ctypes.c_int64 * 10)()
    assert lib.dmad_rs_smooth_votes(None, buf, 0.25, 4, 1, 0, 0, None, cnt, None, None) == -1
    assert b'dmad_rs_smooth_votes' in lib.dmad_last_error()
    assert lib.dmad_m5_rs_smooth_votes(None, buf, 0.25, 4, 0, 0, None, cnt, None, None) == -1
    assert b'dmad_m5_rs_smooth_votes' in lib.dmad_last_error()
    with pytest.raises(_lib.DmadError, match='dmad_m5_rs_smooth_votes'):
        _lib.check(lib.dmad_m5_rs_smooth_votes(None, None, 0.25, 4, 0, 0, None, None, None, None))
    assert list(cnt) == [0] * 10


# ---- route selection ------------------------------------------------------------------------------------------------------------------
class _Engine:
    """stands in for dmad_hip.engine.Engine: what _fused_rs() reads"""
    has_classifier = True
    has_m5 = True
    has_wavenet = False


class _HipClassifier(torch.nn.Module):
    """a HIP-backed classifier as RobustCertificate sees one: bind_engine(), and `engine` in __dict__ once bound"""

    def __init__(self, refuse=False):
        super().__init__()
        self.refuse, self.bound_to = refuse, []
        self.eval()

    def bind_engine(self, engine=None):
        from dmad_hip._lib import DmadError
        self.bound_to.append(engine)
        if engine is not None and self.refuse:
            raise DmadError('this engine already holds different classifier weights')
        self.__dict__['engine'] = engine if engine is not None else _Engine()
        return self


def _certificate(classifier, transform, **kw):
    from robustness_eval.certified_robust import RobustCertificate
    return RobustCertificate(classifier=classifier, transform=transform, denoiser=None, **kw)


def _m5(engine=None):
    from audio_models.M5.M5Net import M5
    m = M5(first_kernel_size=80, n_output=35).eval()
    if engine is not None:
        m.__dict__['engine'] = engine                      # what use_engine() leaves behind
    return m


def test_fused_route_for_the_hip_mel_front_end_and_a_bound_classifier():
    from dmad_hip.transforms import MelSpectrogramDB
    eng = _Engine()
    clf = _HipClassifier()
    clf.bind_engine(eng)
    rc = _certificate(clf, MelSpectrogramDB(eng))
    assert rc._fused_rs() == ('mel', eng) and clf.bound_to == [eng]          # already bound: not bound again
    assert not rc._fused() and rc._fused_spec() is None


def test_unbound_classifier_is_bound_to_the_transforms_engine_first():
    from dmad_hip.transforms import MelSpectrogramDB
    eng = _Engine()
    clf = _HipClassifier()
    assert _certificate(clf, MelSpectrogramDB(eng))._fused_rs() == ('mel', eng) and clf.bound_to == [eng]
    other = _HipClassifier(refuse=True)                     # that engine serves another classifier: an engine of its own, unfused
    assert _certificate(other, MelSpectrogramDB(eng))._fused_rs() is None
    assert other.bound_to == [eng, None] and other.engine is not eng


def test_fused_route_for_the_shims_compose():
    eng = _Engine()

    class Stage:
        def __init__(self, stage):
            self._dmad_stage, self.engine = stage, eng

    class Compose:
        def __init__(self, stages):
            self.transforms = stages

    clf = _HipClassifier()
    assert _certificate(clf, Compose([Stage('mel_power'), Stage('power_to_db')]))._fused_rs() == ('mel', eng)
    assert _certificate(_HipClassifier(), Compose([Stage('kws_mel_power'), Stage('power_to_db')]))._fused_rs() is None
    assert _certificate(_HipClassifier(), Compose([Stage('mel_power')]))._fused_rs() is None


def test_fused_route_for_m5_on_an_engine():
    eng = _Engine()
    assert _certificate(_m5(eng), None)._fused_rs() == ('m5', eng)
    assert _certificate(_m5(eng).train(), None)._fused_rs() is None            # the module's own layers run in training mode


def test_generic_route_is_kept():
    from dmad_hip.transforms import MelSpectrogramDB
    eng = _Engine()
    plain = torch.nn.Linear(4, 4).eval()
    assert _certificate(plain, MelSpectrogramDB(eng))._fused_rs() is None       # a user's torch module
    assert _certificate(plain, None)._fused_rs() is None
    assert _certificate(_m5(), None)._fused_rs() is None                        # a default M5: nobody called use_engine()
    assert _certificate(_m5(eng), MelSpectrogramDB(eng))._fused_rs() is None    # M5 has no bind_engine: not a spectrogram classifier
    foreign = torch.nn.Identity()
    clf = _HipClassifier()
    assert _certificate(clf, foreign)._fused_rs() is None and clf.bound_to == []   # a foreign transform; nothing was bound for it
    assert _certificate(_HipClassifier(), None)._fused_rs() is None             # a spectrogram classifier without its front-end
    from robustness_eval.certified_robust import RobustCertificate
    assert RobustCertificate(clf, MelSpectrogramDB(eng), denoiser=object())._fused_rs() is None     # a denoiser: not this route


class _OnDevice(torch.Tensor):
    """a host tensor that says it is on the GPU: smooth_predict asks before it selects a route"""
    is_cuda = property(lambda self: True)


def test_smooth_predict_takes_the_route_it_selected():
    """smooth_predict hands the shard [lo, hi) and the seed to the selected route: device noise in one call, torch_cpu noise batch by
    batch as `delta`; for a clip on the CPU (no engine can serve it) the host loop is kept."""
    calls = []

    class Eng(_Engine):
        def m5_rs_smooth_votes(self, x, sigma, n, seed=0, sample0=0, delta=None, counts=None):
            calls.append((n, seed, sample0, None if delta is None else tuple(delta.shape)))
            c = torch.zeros(35, dtype=torch.int64) if counts is None else counts
            c[3] += n
            return c, None

    x = torch.zeros(1, 16000).as_subclass(_OnDevice)
    rc = _certificate(_m5(Eng()), None, seed=4)
    counts = rc.smooth_predict(x, num_sampling=37, sigma=0.5, batch_size=16)
    assert counts[3] == 37 and int(counts.sum()) == 37 and calls == [(37, 4 * 1000003, 0, None)] and rc._last is None
    calls.clear()
    rc = _certificate(_m5(Eng()), None, noise_source='torch_cpu')
    counts = rc.smooth_predict(x, num_sampling=37, sigma=0.5, batch_size=16)
    assert counts[3] == 37 and calls == [(16, 0, 0, (16, 1, 16000)), (16, 0, 16, (16, 1, 16000)), (5, 0, 32, (5, 1, 16000))]
    calls.clear()
    counts = rc.smooth_predict(torch.zeros(1, 16000), num_sampling=5, sigma=0.5, batch_size=4)       # a CPU clip: the module itself
    assert int(counts.sum()) == 5 and calls == []
