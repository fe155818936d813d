"""Host side of the baseline waveform defenses (transforms/time_defense.py, transforms/frequency_defense.py, baseline_defense_eval.py):
the 'host' backend against the reference's recorded outputs, the filter designs, the IIR kernel's decomposition restated in numpy, the
fp32 yardstick the GPU bounds are taken from, the host backward, shapes, quirks and the driver's refusals.  No GPU."""
import os

import numpy as np
import pytest
import torch

import wave_defense_cases as wc
from transforms import _wave_design as wd
from transforms.frequency_defense import BPF, DS, LPF, FreqDomainDefense
from transforms.time_defense import AS, MS, TimeDomainDefense

# Recorded sequential-fp32 errors (max |fp32 - float64| on the GPU tests' inputs, printed by test_fp32_error_yardstick) and their ceilings
# (2 x the recorded value: numpy's fp32 arithmetic is IEEE, the value moves only if the inputs do)
YARDSTICK_CEILING = {('LPF', 'forward'): 7.0e-8, ('BPF', 'forward'): 2.6e-5, ('order1', 'forward'): 8.0e-7, ('order8', 'forward'): 5.0e-9,
                     ('LPF', 'adjoint'): 5.0e-7, ('BPF', 'adjoint'): 1.2e-4, ('order1', 'adjoint'): 1.9e-6, ('order8', 'adjoint'): 3.2e-7}


def test_golden_fixture(golden_dir):
    """The 'host' backend reproduces what the reference's time_defense.py gave for three synth clips: MS bit for bit, AS within
    4u sum|terms| (outputs and input gradients)."""
    z = np.load(os.path.join(golden_dir, 'wave_defense.npz'))
    g = torch.from_numpy(z['g'])
    for name, fn in (('AS', AS), ('MS', MS)):
        x = torch.from_numpy(z['x']).requires_grad_(True)
        y = fn(x, backend='host')
        gx, = torch.autograd.grad(y, x, g)
        assert y.shape == x.shape
        if name == 'MS':
            assert np.array_equal(y.detach().numpy(), z['MS_y']) and np.array_equal(gx.numpy(), z['MS_gx'])
        else:
            for got, ref, src in ((y.detach(), z['AS_y'], x.detach()), (gx, z['AS_gx'], g)):
                bound = 4 * wc.U * wd.host_mean(src.abs().double()[:, 0], 3).numpy() + 1e-45
                assert np.all(np.abs(got.numpy()[:, 0].astype(np.float64) - ref[:, 0]) <= bound)


def test_filter_design():
    b, a, N, Wn = wd.butter_lowpass(16000, 4000, 8000, 3, 40)
    assert N == 1 and abs(Wn - 0.50076) < 1e-4 and b.dtype == a.dtype == np.float32 and len(a) == 2
    assert np.abs(np.roots(a.astype(np.float64))).max() < 1.0
    b, a, N, Wn = wd.butter_bandpass(16000, (300, 4000), (50, 8000), 3, 40)
    assert N == 3 and len(a) == 7 and len(b) == 7
    r = np.abs(np.roots(a.astype(np.float64))).max()
    assert abs(r - 0.9467) < 1e-3 and r < 1.0
    r8 = np.abs(np.roots(wc.filters()['order8'][1].astype(np.float64))).max()
    assert abs(r8 - 0.995) < 2e-3 and r8 < 1.0                       # the fp32-rounded order-8 test filter: stable, poles at 0.995


@pytest.mark.parametrize('T', [wc.SEG, 127])
@pytest.mark.parametrize('name', ['LPF', 'BPF', 'order8'])
def test_iir_decomposition(name, T):
    """Segments, carry and re-run, restated in float64 at the kernel's segment length (125) and at one that does not divide 16000,
    equal the sequential filter to 1e-12 (relative to the output peak)."""
    b, a = wc.filters()[name]
    x = np.random.default_rng(5).standard_normal(wc.L) * 0.1
    ref = wc.lfilter64(b, a, x)
    assert (wc.L % T == 0) == (T == wc.SEG)
    assert np.abs(wc.iir_segmented64(b, a, x, T) - ref).max() <= 1e-12 * max(1.0, np.abs(ref).max())


@pytest.mark.parametrize('what', ['forward', 'adjoint'])
@pytest.mark.parametrize('name', ['LPF', 'BPF', 'order1', 'order8'])
def test_fp32_error_yardstick(name, what):
    """Sequential fp32 lfilter against float64 on the GPU tests' own inputs (clips(11); grads(11) reversed for the adjoint).  The GPU
    tests allow 8 x this measured value.  Recorded: LPF 3.45e-08 / 2.48e-07, BPF 1.29e-05 / 5.82e-05, order1 3.87e-07 /
    9.09e-07, order8 2.40e-09 / 1.60e-07 (forward / adjoint; BPF's output peak on these clips is 0.5, its 300 Hz edge puts poles at 0.9467
    and the direct form pays for them)."""
    err = wc.iir_fp32_error(name, what)
    print('fp32 sequential error %s %s: %.3e' % (name, what, err))
    assert 0.0 < err <= YARDSTICK_CEILING[(name, what)]


def test_host_backward():
    b, a = wc.filters()['BPF']
    x = torch.randn(2, 64, dtype=torch.float64, generator=torch.Generator().manual_seed(0)).requires_grad_(True)
    assert torch.autograd.gradcheck(lambda v: wd.HostIIR.apply(v, b, a), (x,))
    assert torch.autograd.gradcheck(lambda v: DS(v, backend='host'), (x,))
    # the clamp's mask: no gradient comes back from an output sample that left [-1, 1]
    lb, la = wc.filters()['LPF']
    big = torch.full((1, 64), 1.1, dtype=torch.float64).requires_grad_(True)          # 0.9 * 1.1 <= 1: the [-1, 1] range; the DC gain is 1
    u = torch.from_numpy(wc.lfilter64(lb, la, big.detach().numpy()))
    assert int((u > 1).sum()) > 32
    y = LPF(big, backend='host')
    g = torch.randn(1, 64, dtype=torch.float64, generator=torch.Generator().manual_seed(1))
    gx, = torch.autograd.grad(y, big, g)
    assert torch.equal(y.detach(), u.clamp(-1, 1))
    assert torch.allclose(gx, torch.from_numpy(wc.lfilter64(lb, la, (g * (u <= 1)).numpy()[:, ::-1])[:, ::-1].copy()), atol=1e-15)


def test_ds_kernel_geometry():
    dk, dw, do, dn = wd.sinc_resample_kernel(16000, 8000)
    uk, uw, uo, un = wd.sinc_resample_kernel(8000, 16000)
    assert dk.shape == (1, 28) and (dw, do, dn) == (13, 2, 1) and dk.dtype == np.float32
    assert uk.shape == (2, 15) and (uw, uo, un) == (7, 1, 2) and uk.dtype == np.float32
    assert wd.resample_length(16000, do, dn) == 8000 and wd.resample_length(8000, uo, un) == 16000
    t = torch.arange(16000, dtype=torch.float64) / 16000
    x = torch.sin(2 * np.pi * 1000 * t).float()
    y = DS(x, backend='host')
    assert y.shape == x.shape
    gain = float(y[200:-200].abs().max() / x[200:-200].abs().max())
    assert abs(gain - 1.0) < 0.01


@pytest.mark.parametrize('fn', [AS, MS, DS, LPF, BPF])
def test_shapes(fn):
    x = torch.from_numpy(wc.clips(2).copy()) * 0.5
    rows = fn(x, backend='host')
    assert rows.shape == (2, wc.L) and rows.dtype == torch.float32
    # (F.conv1d on the CPU may pick another algorithm for another batch size: close, not equal)
    assert fn(x[0], backend='host').shape == (wc.L,) and torch.allclose(fn(x[0], backend='host'), rows[0], atol=1e-6)
    assert fn(x.unsqueeze(1), backend='host').shape == (2, 1, wc.L) and torch.allclose(fn(x.unsqueeze(1), backend='host')[:, 0], rows, atol=1e-6)
    with pytest.raises(NotImplementedError, match='Audio Shape Error'):
        fn(x.view(2, 1, 1, wc.L), backend='host')


def test_quirks():
    x = torch.from_numpy(wc.clips(2).copy())
    # MS pads with zeros: the first output of a clip that starts at 0.4 is median(0, 0.4, 0.4), not a replicated edge
    edge = torch.full((1, 16), 0.4)
    edge[0, 0] = 0.9
    assert float(MS(edge, backend='host')[0, 0]) == pytest.approx(0.4) and float(MS(edge * -1, backend='host')[0, 0]) == pytest.approx(-0.4)
    assert float(MS(torch.tensor([[0.9, -0.4, 0.1]]), backend='host')[0, 0]) == 0.0                      # median(pad 0, 0.9, -0.4)
    # the clamp range: [-1, 1] while 0.9 max <= 1 and 0.9 min >= -1, the int16 range otherwise
    loud = x * (1.05 / x.abs().max())
    assert float(LPF(loud * 4, backend='host').abs().max()) > 1.0
    assert float(LPF(loud, backend='host').abs().max()) <= 1.0
    pcm = x * 2 ** 15
    y = BPF(pcm, backend='host')
    assert float(y.abs().max()) > 100.0 and float(y.max()) <= 2 ** 15 - 1 and float(y.min()) >= -2 ** 15
    # LPF's ws = 8000 at fs = 16000 is ws = 1.0: scipy accepts it and the order stays 1
    assert wd.butter_lowpass(16000, 4000, 8000, 3, 40)[2] == 1
    # the default backend without CUDA input is the host one
    assert torch.equal(AS(x), AS(x, backend='host'))
    with pytest.raises(ValueError, match='backend'):
        AS(x, backend='cuda')


def test_classes():
    x = torch.from_numpy(wc.clips(2).copy())
    names = {'AS': 'Average_Smoothing', 'MS': 'Median_Smoothing', 'DS': 'Down_Sampling', 'LPF': 'Low_Pass_Filter', 'BPF': 'Band_Pass_Filter'}
    for k, fn in (('AS', AS), ('MS', MS), ('DS', DS), ('LPF', LPF), ('BPF', BPF)):
        d = (TimeDomainDefense if k in ('AS', 'MS') else FreqDomainDefense)(k, backend='host')
        assert d._get_name() == names[k] and torch.equal(d(x), fn(x, backend='host'))
    for cls in (TimeDomainDefense, FreqDomainDefense):
        with pytest.raises(NotImplementedError, match='Unknown defense type: XX!'):
            cls('XX')(x)
        with pytest.raises(NotImplementedError, match='Unknown defense type: XX!'):
            cls('XX')._get_name()
    assert TimeDomainDefense('AT')._get_name() == 'Audio_Turbulence'
    with pytest.raises(NotImplementedError, match='not provided'):
        TimeDomainDefense('AT')(x)


def test_driver_flags_and_refusals():
    import adaptive_attack_eval
    import baseline_defense_eval as drv
    import black_box_attack_eval
    import siren_attack_eval
    args = drv.build_parser().parse_args(['--attack', 'CW', '--defense', 'BPF'])
    want = dict(data_path='datasets/speech_commands/test', classifier_model='resnext29_8_64', classifier_type='vanilla', classifier_input='mel32',
                num_per_class=10, sample_step=1, t=1, t_delta=15, rand_t=False, diffusion_type='ddpm', score_type='guided_diffusion', use_bm=False,
                bound_norm='linf', eps=65, max_iter_1=10, max_iter_2=0, eot_attack_size=1, eot_defense_size=1, verbose=1,
                dataload_workers_nums=8, batch_size=20, gpu=0, save_path=None, defense_backend='hip')
    assert {k: getattr(args, k) for k in want} == want
    assert drv.ATTACKS == ['CW', 'FAKEBOB', 'SirenAttack'] and drv.DEFENSES == ['AS', 'MS', 'DS', 'LPF', 'BPF']
    drv.check_supported(args)
    owner = {'CW': 'adaptive_attack_eval.py', 'FAKEBOB': 'black_box_attack_eval.py', 'SirenAttack': 'siren_attack_eval.py'}
    for attack in drv.ATTACKS:
        for d in ('None', 'Diffusion', 'Diffusion-Spec'):
            with pytest.raises(NotImplementedError, match=r'--defense %s: %s runs it' % (d, owner[attack].replace('.', r'\.'))):
                drv.check_supported(drv.build_parser().parse_args(['--attack', attack, '--defense', d]))
    for d in ('FeCo', 'DefenseGAN'):
        with pytest.raises(NotImplementedError, match='--defense %s needs .* does not provide' % d):
            drv.check_supported(drv.build_parser().parse_args(['--defense', d]))
    for a in ('Qin-I', 'Kenansville'):
        with pytest.raises(NotImplementedError, match='--attack %s: this driver runs CW, FAKEBOB and SirenAttack' % a):
            drv.check_supported(drv.build_parser().parse_args(['--attack', a, '--defense', 'AS']))
    with pytest.raises(NotImplementedError, match='max_iter_2'):
        drv.check_supported(drv.build_parser().parse_args(['--defense', 'AS', '--max_iter_2', '1']))
    # the three existing drivers keep refusing the five defenses, by name, and now name this driver
    for other, attack in ((adaptive_attack_eval, 'CW'), (black_box_attack_eval, 'FAKEBOB'), (siren_attack_eval, 'SirenAttack')):
        for d in drv.DEFENSES:
            with pytest.raises(NotImplementedError, match=r'--defense %s .*baseline_defense_eval\.py' % d):
                other.check_supported(other.build_parser().parse_args(['--attack', attack, '--defense', d]))
    d = drv.build_defender(drv.build_parser().parse_args(['--defense', 'MS', '--defense_backend', 'host']))
    assert isinstance(d, TimeDomainDefense) and d.backend == 'host' and d.engine is None
    d = drv.build_defender(drv.build_parser().parse_args(['--defense', 'DS']), engine='E')
    assert isinstance(d, FreqDomainDefense) and d.backend == 'hip' and d.engine == 'E'
