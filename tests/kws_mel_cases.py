"""The keyword spotter's mel front-end (torchaudio MelSpectrogram(sample_rate=16000, n_mels=32) then AmplitudeToDB('power')) and its
whole backward written out by hand in the matrix form the engine's kernels use (csrc/kws_mel.hip): reflect map, windowed DFT matrix,
|.|^2, htk filterbank, clamp and log, and back through each of them to the fold of the reflect padding.  No autograd, no FFT:
tests/test_kws_mel_cpu.py proves it against torch.stft-based float64 autograd, and the GPU tests use it as their reference.  Also the
inputs of those tests (rows), built once per length."""
import functools
import os
import wave

import numpy as np
import torch

N_FFT, HOP, BINS, MELS = 400, 200, 201, 32
CASES = (800, 801, 999, 1000, 1237, 6600, 16000)
TILE = 8                                             # kMelTile of csrc/kws_mel.h: frames of one forward workgroup
TILE_CASES = tuple(HOP * (t - 1) + 41 for t in (TILE - 1, TILE, TILE + 1))      # T one below, at and one above the tile
CAP = 128799                                         # the longest clip the wave exports take (T = 644)


def frames_of(L):
    return 1 + L // HOP


def reflect_index(L):
    """sample index of every padded position p < L + 400: |p - 200| on the left, 2 (L - 1) - (p - 200) on the right"""
    q = np.arange(L + 2 * HOP) - HOP
    q = np.where(q < 0, -q, q)
    return np.where(q >= L, 2 * (L - 1) - q, q)


@functools.lru_cache(maxsize=None)
def constants():
    """float64: the DFT matrix [402][400] (201 rows window * cos, 201 rows -window * sin) and the htk filterbank [32][201]"""
    n = np.arange(N_FFT)
    win = 0.5 - 0.5 * np.cos(2.0 * np.pi * n / N_FFT)                       # periodic Hann
    ang = 2.0 * np.pi * ((np.arange(BINS)[:, None] * n[None, :]) % N_FFT) / N_FFT
    A = np.concatenate([win * np.cos(ang), -win * np.sin(ang)])
    mel = np.linspace(0.0, 2595.0 * np.log10(1.0 + 8000.0 / 700.0), MELS + 2)
    pts = 700.0 * (10.0 ** (mel / 2595.0) - 1.0)
    f = np.linspace(0.0, 8000.0, BINS)
    down = (f[None, :] - pts[:-2, None]) / (pts[1:-1, None] - pts[:-2, None])
    up = (pts[2:, None] - f[None, :]) / (pts[2:, None] - pts[1:-1, None])
    return torch.from_numpy(A), torch.from_numpy(np.maximum(0.0, np.minimum(down, up)))


def mel_walk(x, g=None, dtype=torch.float64, window=None, fb=None, fold=True):
    """x [B,L] (or [B,1,L]) -> every stage of the front-end in `dtype`, the constants computed in float64 and rounded once; with g
    [B,32,T] also every stage of the backward.  window / fb / fold: the deliberate breaks of the margin measurements (another window
    [400], another filterbank [32][201], the fold of the reflected samples dropped)."""
    x = x.reshape(x.shape[0], -1).to(dtype)
    B, L = x.shape
    T = frames_of(L)
    A64, fb64 = constants()
    if window is not None:
        n = np.arange(N_FFT)
        hann = torch.from_numpy(0.5 - 0.5 * np.cos(2.0 * np.pi * n / N_FFT))
        A64 = A64 / torch.where(hann == 0, torch.ones_like(hann), hann) * torch.as_tensor(window, dtype=torch.float64)
    A = A64.to(dtype)
    F = (fb64 if fb is None else torch.as_tensor(fb, dtype=torch.float64)).to(dtype)
    idx = torch.from_numpy(reflect_index(L))
    out = {'T': T}
    padded = x[:, idx]                                                      # [B, L + 400]
    fr = padded.unfold(1, N_FFT, HOP)                                       # [B, T, 400]
    assert fr.shape[1] == T
    D = fr @ A.T                                                            # [B, T, 402]
    re, im = D[..., :BINS], D[..., BINS:]
    power = re * re + im * im                                               # [B, T, 201]
    mel = (power @ F.T).transpose(1, 2)                                     # [B, 32, T]
    db = 10.0 * torch.log10(torch.clamp(mel, min=1e-10))
    out.update(padded=padded, frames=fr, D=D, power=power, mel=mel, db=db)
    if g is None:
        return out
    g = g.reshape(B, MELS, T).to(dtype)
    g_mel = torch.where(mel > 1e-10, g * (10.0 / np.log(10.0)) / torch.clamp(mel, min=1e-10), torch.zeros_like(mel))
    g_power = g_mel.transpose(1, 2) @ F                                     # [B, T, 201]
    g_D = torch.cat([2.0 * re * g_power, 2.0 * im * g_power], dim=-1)       # [B, T, 402]
    g_fr = g_D @ A                                                          # [B, T, 400]
    g_pad = torch.zeros(B, L + 2 * HOP, dtype=dtype)
    for t in range(T):                                                      # overlap-add, frames ascending
        g_pad[:, t * HOP:t * HOP + N_FFT] += g_fr[:, t]
    g_x = g_pad[:, HOP:HOP + L].clone()                                     # direct
    if fold:                                                                # the adjoint of the reflect padding, left then right
        g_x[:, 1:HOP + 1] += g_pad[:, :HOP].flip(1)
        g_x[:, L - HOP - 1:L - 1] += g_pad[:, L + HOP:].flip(1)
    out.update(g_mel=g_mel, g_power=g_power, g_D=g_D, g_frames=g_fr, g_padded=g_pad, g_x=g_x)
    return out


@functools.lru_cache(maxsize=None)
def rows(L, B=3):
    """(x [B,L] float32, g [B,32,T] float32): row 0 noise, row 1 a 440 Hz tone over a little noise (quiet bins, cancellation), row 2
    silence; rows past 2 are more noise"""
    gen = torch.Generator().manual_seed(2300 + L % 100003)
    x = torch.randn(B, L, generator=gen) * 0.1
    if B > 1:
        t = torch.arange(L, dtype=torch.float64) / 16000.0
        x[1] = (0.5 * torch.sin(2.0 * np.pi * 440.0 * t)).float() + 1e-3 * torch.randn(L, generator=gen)
    if B > 2:
        x[2] = 0.0
    g = torch.randn(B, MELS, frames_of(L), generator=gen)
    return x, g


@functools.lru_cache(maxsize=None)
def case(L, B=3):
    """(x, g, the float64 walk, the fp32 walk's own error: absolute in dB / in mel power relative to its largest value / of the
    gradient's maximum, none below one ulp of the largest value) -- computed once and shared"""
    x, g = rows(L, B)
    ref = mel_walk(x, g)
    own = mel_walk(x, g, dtype=torch.float32)
    ulp = 2.0 ** -23
    e_db = max((own['db'].double() - ref['db']).abs().max().item(), ulp * ref['db'].abs().max().item())
    pmax = ref['mel'].abs().max().item()
    e_pow = max((own['mel'].double() - ref['mel']).abs().max().item() / pmax, ulp)
    gmax = ref['g_x'].abs().max().item()
    e_g = max((own['g_x'].double() - ref['g_x']).abs().max().item() / gmax, ulp)
    return x, g, ref, e_db, e_pow, e_g


def write_wav(path, samples, rate=16000):
    with wave.open(str(path), 'wb') as w:
        w.setnchannels(1)
        w.setsampwidth(2)
        w.setframerate(rate)
        w.writeframes((np.asarray(samples) * 32767.0).round().astype('<i2').tobytes())


def make_tree(root, per_class=3, classes=None, lengths=(1600, 2400)):
    """a keyword dataset of 16-bit WAVs under root/<class>/[speaker/]clip_NN.wav, written in a shuffled order"""
    from datasets.qualcomm_kws_dataset import CLASSES
    rng = np.random.RandomState(3)
    for c in classes or CLASSES:
        os.makedirs(os.path.join(root, c, 'speaker'), exist_ok=True)
        for i in rng.permutation(per_class):
            where = os.path.join(root, c, 'speaker' if i % 2 else '', 'clip_%02d.wav' % i)
            write_wav(where, rng.uniform(-0.3, 0.3, rng.randint(lengths[0], lengths[1] + 1)))
    return root
