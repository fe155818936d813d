"""Float64 numpy walk of the masking loss of the imperceptible attack and of its gradient (the reference's
_loss_gradient_masking_threshold / _approximate_power_spectral_density, white_box_attack.py l.606-678), shared by tests/test_qin_cpu.py
(which checks it against torch.autograd in float64) and tests/test_gpu_qin.py (which checks the engine against it).

masking_walk(delta [B, L], theta [B, 1025, F], psd_scale [B], mask=None) -> dict with
  psd   [B, 1025, F]  psd_scale (8/3) / 2048^2 |STFT|^2, STFT the uncentred Hann-windowed frames of delta (window 2048, hop 512)
  mask  [B, 1025, F]  psd > theta (strict: torch's ReLU has gradient 0 at 0), or the mask passed in (`pinned`: a comparison of two
                      gradients must not depend on which side of the hinge a bin within rounding of its threshold falls)
  loss  [B]           mean over (k, f) of mask * (psd - theta)
  g     [B, L]        d sum(loss) / d delta under that mask; samples >= 512 (F - 1) + 2048 lie in no frame: exactly 0
step_ref(x, delta, g_net, alpha, signed_lr, g_theta) is the reference's update (l.569-573) in float64."""
import numpy as np

WIN, HOP, BINS = 2048, 512, 1025
GAIN = (8.0 / 3.0) / (WIN * WIN)


def n_frames(L):
    return (L - WIN) // HOP + 1


def hann():
    return 0.5 - 0.5 * np.cos(2.0 * np.pi * np.arange(WIN) / WIN)


def masking_walk(delta, theta, psd_scale, mask=None):
    delta = np.asarray(delta, np.float64)
    theta = np.asarray(theta, np.float64)
    scale = np.asarray(psd_scale, np.float64).reshape(-1, 1, 1)
    B, L = delta.shape
    F = n_frames(L)
    w = hann()
    idx = HOP * np.arange(F)[:, None] + np.arange(WIN)[None, :]
    S = np.fft.rfft(delta[:, idx] * w, axis=2)                               # [B, F, 1025]
    psd = scale * GAIN * (S.real ** 2 + S.imag ** 2).transpose(0, 2, 1)      # [B, 1025, F]
    if mask is None:
        mask = psd > theta
    mask = np.asarray(mask, bool)
    loss = (mask * (psd - theta)).sum(axis=(1, 2)) / (BINS * F)
    # d loss / d (re, im) = mask 2 (re, im) scale GAIN / (K F); re = sum_n w[n] x[n] cos(2 pi k n / N), im = -sum_n w[n] x[n] sin(.)
    # => d loss / d x[n] = w[n] Re(sum_k (g_re + i g_im)[k] exp(+2 pi i k n / N)), the sum over the 1025 bins only (no Hermitian half)
    G = (mask * (2.0 * scale * GAIN / (BINS * F))).transpose(0, 2, 1) * S    # [B, F, 1025] complex: g_re + i g_im
    full = np.zeros((B, F, WIN), np.complex128)
    full[:, :, :BINS] = G
    gF = w * (np.fft.ifft(full, axis=2).real * WIN)                          # [B, F, 2048]
    g = np.zeros((B, L))
    for f in range(F):
        g[:, HOP * f:HOP * f + WIN] += gF[:, f]
    return {'psd': psd, 'mask': mask, 'loss': loss, 'g': g}


def step_ref(x, delta, g_net, alpha, signed_lr, g_theta):
    x, delta, g_net, g_theta = (np.asarray(a, np.float64) for a in (x, delta, g_net, g_theta))
    d = delta + float(signed_lr) * (g_net + np.asarray(alpha, np.float64).reshape(-1, 1) * g_theta)
    return np.clip(x + d, -1.0, 1.0) - x


def sign_delta(B, L=16000, amplitude=65.0 / 32768.0):
    """the perturbations of the GPU tests: amplitude times random signs, seed b for row b"""
    return np.stack([amplitude * (np.random.RandomState(b).randint(0, 2, L) * 2.0 - 1.0) for b in range(B)]).astype(np.float32)
