"""The WaveNet VJP's C ABI without a GPU: dmad.h declares dmad_reserve_vjp / dmad_wavenet_eps_vjp, the cross-compiled library
exports them, and dmad_hip._lib binds them with their argument types."""
import ctypes
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, 'diffusion-model-for-audio-defense_amd')
LIB = os.path.join(PKG, 'libdmad_hip.so')
NAMES = ('dmad_reserve_vjp', 'dmad_wavenet_eps_vjp')


@pytest.fixture(scope='module')
def lib():
    if not os.path.exists(LIB):
        subprocess.run(['make', '-C', os.path.join(PKG, 'csrc'), '-j4'], check=True)
    return ctypes.CDLL(LIB)


def test_header_declares_the_vjp():
    hdr = re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', 'dmad.h')).read(), flags=re.S)
    assert re.search(r'int\s+dmad_reserve_vjp\s*\(\s*dmad_engine\s*\*\s*e\s*,\s*int32_t\s+max_batch\s*\)\s*;', hdr)
    m = re.search(r'int\s+dmad_wavenet_eps_vjp\s*\(([^)]*)\)\s*;', hdr)
    assert m
    args = [a.strip() for a in m.group(1).split(',')]
    assert [re.sub(r'\s+', ' ', a.rsplit(' ', 1)[0].replace('*', ' *')).strip() for a in args] == [
        'dmad_engine *', 'const float *', 'int32_t', 'int32_t', 'const float *', 'float *', 'float *', 'dmad_stream']


def test_library_exports_the_vjp(lib):
    for name in NAMES:
        assert hasattr(lib, name), name


def test_lib_binds_the_vjp():
    from dmad_hip import _lib
    for name in NAMES:
        assert name in _lib.EXPORTS
    P, i32 = ctypes.c_void_p, ctypes.c_int32
    assert _lib._SIGNATURES['dmad_reserve_vjp'] == (ctypes.c_int, [P, i32])
    assert _lib._SIGNATURES['dmad_wavenet_eps_vjp'] == (ctypes.c_int, [P, P, i32, i32, P, P, P, P])
