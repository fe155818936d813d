"""The FFT form of the Kenansville attack (behaviour of the reference's robustness_eval/_KenanFFT.py: fft_compression l.57-82 and
atk_bst_fft l.180-247; "Hear 'No Evil', See 'Kenansville': Efficient and Transferable Black-Box Attacks on Speech Recognition and Voice
Identification Systems", IEEE S&P 2021), restated for this package.

Per batch of clips [n, 1, L]: the bins of the clip's real FFT whose magnitude is below a per-clip factor are zeroed, the inverse
transform is shown to the system, and the factor is bisected per clip between 0 and the largest |FFT| of the clip:
  * the first factor is half of that maximum;
  * a clip that is misclassified (classified as its label, when targeted) at a factor keeps that perturbed clip, and its upper bound
    becomes the factor; otherwise the lower bound does; the next factor is |(lower + upper) / 2|;
  * always `max_iter` iterations (the reference's early_stop flag is accepted and unused, as there);
  * the result is, per clip, the LAST perturbed clip that succeeded (the one with the smallest successful factor seen) or the input, and
    `succ` says whether any iteration succeeded.
`backend='torch'` is the reference's operators in the reference's order: torch.fft.fft for the maximum, torch.fft.rfft, the masked
assignment and torch.fft.irfft per iteration, the per-clip host loop for the bisection (tests/golden/kenansville.npz is recorded from the
reference and judges this path bit for bit).  `backend='device'` takes ONE dmad_wave_rfft per batch -- the clips do not
change between iterations -- and per iteration one dmad_wave_irfft_threshold, the system's scores, an arg-max and one
dmad_kenan_update; the bounds, the factors, the kept clips and `succ` stay on the device and only `succ` is read back, once, at the
end.  The bisection statements are torch's fp32 statements bit for bit; the transforms agree with torch.fft within fp32 rounding, so a
bin whose magnitude is within that rounding of a factor may fall on the other side.
`trace`, when a list, receives per iteration (factors, predictions) as they were when the system was asked."""
import torch


def fft_compression(clips, factor):
    """reference l.57-82: clips [n, 1, L], factor [n] -> the clips with every bin |X| < factor zeroed"""
    bins = torch.fft.rfft(clips, dim=2)
    bins[bins.abs() < factor.unsqueeze(1).unsqueeze(2)] = 0
    return torch.fft.irfft(bins, dim=2)


def atk_bst_fft(data, labels_in, targeted, scores_of, max_iter, verbose=0, backend='torch', engine=None, trace=None):
    """data [n, 1, L], labels_in [n]; scores_of(x [n, 1, L]) -> scores [n, C].  Returns (clips [n, 1, L], succ: list of n bools)."""
    if backend == 'device':
        return _atk_bst_fft_device(data, labels_in, targeted, scores_of, max_iter, verbose, engine, trace)
    n = data.shape[0]
    device = data.device
    kept_clips = data.clone()
    lower = torch.tensor([0.] * n).to(device)
    upper = torch.fft.fft(data, dim=2).abs().max(dim=2)[0].view(-1)
    factor = upper / 2
    succ = [False] * n
    for itr in range(max_iter):
        perturbed = fft_compression(data.clone(), factor)
        scores = scores_of(perturbed)
        predicted_p = scores.max(1, keepdim=True)[1]
        if trace is not None:
            trace.append((factor.clone(), predicted_p.view(-1).clone()))
        if verbose:
            print('Iter: {} ori: {} atk: {} f: {}'.format(itr + 1, labels_in, predicted_p, factor))
        for i in range(n):
            if (labels_in[i] != predicted_p[i] and not targeted) or (labels_in[i] == predicted_p[i] and targeted):
                kept_clips[i, ...] = perturbed[i, ...]
                upper[i] = factor[i]
                factor[i] = ((lower[i] + upper[i]) / 2).abs()
                succ[i] = True
            else:
                lower[i] = factor[i]
                factor[i] = ((lower[i] + upper[i]) / 2).abs()
    return kept_clips, succ


def _atk_bst_fft_device(data, labels_in, targeted, scores_of, max_iter, verbose, engine, trace):
    n, n_channels, L = data.shape
    x = data[:, 0].float().contiguous()
    labels = torch.as_tensor(labels_in, device=x.device).long().contiguous()
    spec, upper = engine.wave_rfft(x)                        # once: the clips do not change between iterations
    lower = torch.zeros_like(upper)
    factor = upper / 2
    best = x.clone()
    succ = torch.zeros((n,), device=x.device, dtype=torch.int32)
    perturbed = kept = None
    for itr in range(max_iter):
        perturbed, kept = engine.wave_irfft_threshold(spec, factor, perturbed, kept)
        scores = scores_of(perturbed.view(n, 1, L))
        predicted = scores.max(1)[1].long()
        if trace is not None:
            trace.append((factor.clone(), predicted.clone()))
        if verbose:
            print('Iter: {} ori: {} atk: {} f: {}'.format(itr + 1, labels, predicted, factor))
        engine.kenan_update(predicted, labels, targeted, perturbed, best, lower, upper, factor, succ)
    return best.view(n, 1, L).to(data.dtype), succ.cpu().bool().tolist()
