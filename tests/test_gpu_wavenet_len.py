"""Clips of any length on the engine's exact-fp32 DiffWave path (dmad_wavenet_eps_len, dmad_wavenet_eps_vjp_len, dmad_philox_normal_len,
dmad_diffuse_len, dmad_ddpm_step_len, dmad_ddpm_purify_len; DiffWave(.., any_length=True); the keyword-spotting driver's native-length
Diffusion row): against the float64 oracle of tests/wavenet_len_cases.py, whose cases tests/test_wavenet_len_cpu.py proves kink-free,
and bit for bit against the fixed-length twins, a fresh engine, an engine of another clip_len, explicit noise and single rows.

Tolerances are the project's own: FP32_TOL = 2e-5 for eps (tests/test_gpu_parity.py), VJP_TOL = 1e-4 for g_x against float64 autograd
(tests/test_gpu_wavenet_vjp.py), 1e-3 for the hip branch against the torch branch through a model (the same file).

The padding invariant (test_padding_invariant): a call at len must find zeros in rows [len, longest call since) of every zero-padded
map, because the dilated taps reach past the clip's end; the engine clears that band before a shorter call."""
import ctypes
import json
import os

import numpy as np
import pytest
import torch

import kws_cases as kc
import kws_mel_cases as mc
import wavenet_len_cases as wc
from dmad_hip import synth

pytestmark = pytest.mark.gpu

SEED, KEY = 3, 40                       # the Philox keys of the twin test in test_gpu_parity.py (seed of its purifier, _draws = 40)


def new_engine(geom='small', clip_len=None, max_batch=None, precision=None, vjp=0):
    from dmad_hip import engine as E
    G = wc.GEOMETRY[geom]
    eng = E.Engine(wavenet_config=wc.wavenet_config(geom), clip_len=clip_len or G['clip_len'], max_batch=max_batch or G['max_batch'],
                   precision=E.FP32 if precision is None else precision, with_classifier=False,
                   **({'recheck_batch': max_batch or G['max_batch']} if precision == E.EXACT else {}))
    eng.load_wavenet(wc.state_dict(geom))
    if vjp:
        eng.reserve_vjp(vjp)
    return eng


@pytest.fixture(scope='module')
def small():
    eng = new_engine('small', vjp=3)
    yield eng
    eng.close()


@pytest.fixture(scope='module')
def full():
    eng = new_engine('full', vjp=1)
    yield eng
    eng.close()


def noise(B, n, seed, scale=0.5):
    return (torch.randn((B, n), generator=torch.Generator().manual_seed(seed)) * scale).cuda()


def coefficients(ts=2):
    """(t*, c_a, c_b, c_eps[], c_div[], c_sig[]) of DiffWave.forward at reverse_timestep ts"""
    from diffusion_models.diffwave_ddpm import DiffWave
    from oracle import dmad_oracle as orc
    return DiffWave(None, orc.calc_diffusion_hyperparams(**synth.DIFFUSION_CONFIG), reverse_timestep=ts).purify_coefficients()


# ---- 1, 2. against the float64 oracle ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('case', wc.EPS_CASES, ids=wc.case_id)
def test_eps_against_the_oracle(case, request):
    eng = request.getfixturevalue(case[0])
    x, _ = wc.inputs(case)
    got = eng.wavenet_eps_len(x.cuda(), wc.GEOMETRY[case[0]]['t']).cpu().numpy()
    err = wc.relmax(got, wc.reference(case)[0])
    print('%s: eps vs float64 oracle %.2e (FP32_TOL %.0e)' % (wc.case_id(case), err, wc.FP32_TOL))
    assert got.shape == (case[1], case[2]) and np.isfinite(got).all() and err <= wc.FP32_TOL


@pytest.mark.parametrize('case', wc.VJP_CASES, ids=wc.case_id)
def test_vjp_against_float64_autograd(case, request):
    eng = request.getfixturevalue(case[0])
    x, g = wc.inputs(case)
    t = wc.GEOMETRY[case[0]]['t']
    gx, eps = eng.wavenet_eps_vjp_len(x.cuda(), t, g.cuda(), want_eps=True)
    err = wc.relmax(gx.cpu().numpy(), wc.reference(case)[1])
    print('%s: g_x vs float64 autograd %.2e (VJP_TOL %.0e)' % (wc.case_id(case), err, wc.VJP_TOL))
    assert gx.shape == (case[1], case[2]) and bool(torch.isfinite(gx).all()) and err <= wc.VJP_TOL
    assert torch.equal(eps, eng.wavenet_eps_len(x.cuda(), t))


# ---- 3. len == clip_len: the twins, bit for bit ----------------------------------------------------------------------------------------
def test_clip_len_equals_the_twins(small):
    from dmad_hip import engine as E
    eng, L = small, small.L
    x, g = noise(3, L, 21), noise(3, L, 22, 1.0)
    ts, c_a, c_b, c_eps, c_div, c_sig = coefficients()
    assert torch.equal(eng.wavenet_eps_len(x, 12), eng.wavenet_eps(x, 12))
    gx, eps = eng.wavenet_eps_vjp(x, 12, g, want_eps=True)
    gxl, epsl = eng.wavenet_eps_vjp_len(x, 12, g, want_eps=True)
    assert torch.equal(gxl, gx) and torch.equal(epsl, eps)
    z = noise(3, L, 23, 1.0)
    for zz in (None, z):
        assert torch.equal(eng.diffuse_len(x, c_a, c_b, zz, seed=SEED, sample0=KEY), eng.diffuse(x, c_a, c_b, zz, seed=SEED, sample0=KEY))
        a, b = x.clone(), x.clone()
        eng.ddpm_step_len(a, 1, c_eps[1], c_div[1], c_sig[1], zz, seed=SEED, sample0=KEY)
        eng.ddpm_step(b, 1, c_eps[1], c_div[1], c_sig[1], zz, seed=SEED, sample0=KEY)
        assert torch.equal(a, b)
    assert torch.equal(eng.ddpm_purify_len(x, ts, c_a, c_b, c_eps, c_div, c_sig, seed=SEED, sample0=KEY),
                       eng.ddpm_purify(x, ts, c_a, c_b, c_eps, c_div, c_sig, seed=SEED, sample0=KEY))
    assert torch.equal(eng.philox_normal(SEED, KEY, 7, 3, length=L), eng.philox_normal(SEED, KEY, 7, 3))
    # an exact-vote engine serves the same exports on its fp32 path, whatever its mode
    ex = new_engine('small', precision=E.EXACT, vjp=3)
    assert torch.equal(ex.wavenet_eps_len(x, 12), ex.wavenet_eps_path(x, 12, E.WAVE_FP32))
    gx, eps = ex.wavenet_eps_vjp(x, 12, g, want_eps=True)
    gxl, epsl = ex.wavenet_eps_vjp_len(x, 12, g, want_eps=True)
    assert torch.equal(gxl, gx) and torch.equal(epsl, eps)
    short = x[:, :1021].contiguous()
    assert torch.equal(ex.wavenet_eps_len(short, 12), eng.wavenet_eps_len(short, 12))
    ex.close()


# ---- 4. the padding invariant -----------------------------------------------------------------------------------------------------------
def test_padding_invariant(small):
    """A clip_len call on random data leaves rows [129, 2048) of every map dirty; the call at 129 that follows must give the bits of a
    fresh engine's first call, for eps and for the VJP (whose maps are the saved streams, the three gradient regions and g_H), for one clip
    and for the whole batch; then 1021 after 129 (the maps grow again over a band that was cleared) likewise."""
    eng, L = small, small.L
    x, g = noise(3, L, 31, 1.0), noise(3, L, 32, 1.0)
    eng.wavenet_eps(x, 12)
    eng.wavenet_eps_vjp(x, 12, g)
    for n in (129, 1021):
        xs, gs = x[:, :n].contiguous(), g[:, :n].contiguous()
        fresh = new_engine('small', vjp=3)
        want_eps = fresh.wavenet_eps_len(xs, 12)
        want_gx, want_eps2 = fresh.wavenet_eps_vjp_len(xs, 12, gs, want_eps=True)
        fresh.close()
        assert torch.equal(want_eps, want_eps2)
        if n == 129:                                            # one clip first: the other clips' bands must be clean for the batch after it
            assert torch.equal(eng.wavenet_eps_len(xs[:1], 12), want_eps[:1]), n
            assert torch.equal(eng.wavenet_eps_vjp_len(xs[:1], 12, gs[:1]), want_gx[:1]), n
        assert torch.equal(eng.wavenet_eps_len(xs, 12), want_eps), n
        got_gx, got_eps = eng.wavenet_eps_vjp_len(xs, 12, gs, want_eps=True)
        assert torch.equal(got_gx, want_gx) and torch.equal(got_eps, want_eps), n


# ---- 5. the same bits across engine lengths ---------------------------------------------------------------------------------------------
def test_same_bits_as_an_engine_of_that_clip_len(small):
    x = noise(3, 384, 41)
    other = new_engine('small', clip_len=384)
    want = other.wavenet_eps(x, 12)
    other.close()
    assert torch.equal(small.wavenet_eps_len(x, 12), want)


# ---- 6. noise ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('n', [1, 2, 3, 5, 1021, 2048])
def test_noise_is_a_prefix(small, n):
    eng = small
    ts, c_a, c_b, c_eps, c_div, c_sig = coefficients()
    for stream in (0xD1FF, 2, 7):
        assert torch.equal(eng.philox_normal(SEED, KEY, stream, 3, length=n), eng.philox_normal(SEED, KEY, stream, 3)[:, :n])
    x = noise(3, n, 50 + n)
    z0 = eng.philox_normal(SEED, KEY, 0xD1FF, 3)[:, :n].contiguous()
    assert torch.equal(eng.diffuse_len(x, c_a, c_b, None, seed=SEED, sample0=KEY), eng.diffuse_len(x, c_a, c_b, z0))
    z1 = eng.philox_normal(SEED, KEY, 1 + 1, 3)[:, :n].contiguous()
    a, b = x.clone(), x.clone()
    eng.ddpm_step_len(a, 1, c_eps[1], c_div[1], c_sig[1], None, seed=SEED, sample0=KEY)
    eng.ddpm_step_len(b, 1, c_eps[1], c_div[1], c_sig[1], z1)
    assert torch.equal(a, b) and not torch.equal(a, x)
    out = eng.ddpm_purify_len(x, ts, c_a, c_b, c_eps, c_div, c_sig, seed=SEED, sample0=KEY)
    step = eng.diffuse_len(x, c_a, c_b, None, seed=SEED, sample0=KEY)
    eng.ddpm_step_len(step, 1, c_eps[1], c_div[1], c_sig[1], None, seed=SEED, sample0=KEY)
    eng.ddpm_step_len(step, 0, c_eps[0], c_div[0], 0.0, None, seed=SEED, sample0=KEY)
    assert torch.equal(out, step) and bool(torch.isfinite(out).all())


# ---- 7. batch independence --------------------------------------------------------------------------------------------------------------
def test_batch_independence(small):
    eng, n = small, 1021
    x, g = noise(3, n, 61), noise(3, n, 62, 1.0)
    ts, c_a, c_b, c_eps, c_div, c_sig = coefficients()
    eps = eng.wavenet_eps_len(x, 12)
    gx = eng.wavenet_eps_vjp_len(x, 12, g)
    pur = eng.ddpm_purify_len(x, ts, c_a, c_b, c_eps, c_div, c_sig, seed=SEED, sample0=KEY)
    for b in range(3):
        r = slice(b, b + 1)
        assert torch.equal(eng.wavenet_eps_len(x[r], 12), eps[r]), b
        assert torch.equal(eng.wavenet_eps_vjp_len(x[r], 12, g[r]), gx[r]), b
        assert torch.equal(eng.ddpm_purify_len(x[r], ts, c_a, c_b, c_eps, c_div, c_sig, seed=SEED, sample0=KEY + b), pur[r]), b


# ---- 8. refusals ------------------------------------------------------------------------------------------------------------------------
def test_refusals(small):
    from dmad_hip import engine as E
    from dmad_hip._lib import DmadError, check
    eng, L = small, small.L
    ts, c_a, c_b, c_eps, c_div, c_sig = coefficients()
    x = noise(2, 1021, 71)
    before, bytes_before = eng.wavenet_eps_len(x, 12), eng.device_bytes()
    for n in (0, L + 1):
        bad = torch.zeros((1, n), device='cuda')
        calls = (lambda: eng.wavenet_eps_len(bad, 12), lambda: eng.wavenet_eps_vjp_len(bad, 12, bad),
                 lambda: eng.diffuse_len(bad, c_a, c_b, None), lambda: eng.ddpm_step_len(bad.clone(), 1, c_eps[1], c_div[1], c_sig[1], None),
                 lambda: eng.ddpm_purify_len(bad, ts, c_a, c_b, c_eps, c_div, c_sig), lambda: eng.philox_normal(1, 2, 3, 1, length=n))
        for call in calls:
            with pytest.raises(DmadError, match=r'len %d outside \[1, clip_len=%d\]' % (n, L)):
                call()
    x4 = noise(4, 1021, 73)                                     # B is checked as in the twin: 4 > max_batch 3 (the method itself walks passes)
    with pytest.raises(DmadError, match='batch 4'):
        check(eng.lib.dmad_wavenet_eps_len(eng._h, ctypes.c_void_p(x4.data_ptr()), 12, 4, 1021, ctypes.c_void_p(torch.empty_like(x4).data_ptr()), None))
    with pytest.raises(AssertionError):                         # the fixed-length methods keep refusing other lengths
        eng.wavenet_eps(x, 12)
    bf = new_engine('small', precision=E.BF16)
    for call in (lambda: bf.wavenet_eps_len(x, 12), lambda: bf.diffuse_len(x, c_a, c_b, None), lambda: bf.philox_normal(1, 2, 3, 1, length=5),
                 lambda: bf.ddpm_purify_len(x, ts, c_a, c_b, c_eps, c_div, c_sig)):
        with pytest.raises(DmadError, match='BF16'):
            call()
    bf.close()
    # the engine is as usable as before, and a run of _len calls allocates nothing
    assert torch.equal(eng.wavenet_eps_len(x, 12), before)
    eng.wavenet_eps_vjp_len(x, 12, x)
    eng.ddpm_purify_len(x[:, :5].contiguous(), ts, c_a, c_b, c_eps, c_div, c_sig)
    eng.ddpm_purify_len(noise(3, L, 72), ts, c_a, c_b, c_eps, c_div, c_sig)
    eng.philox_normal(1, 2, 3, 3, length=7)
    assert eng.device_bytes() == bytes_before


# ---- 9. through the model ---------------------------------------------------------------------------------------------------------------
def test_through_the_model(small, tmp_path):
    from diffusion_models.diffwave_ddpm import create_diffwave_model
    cfg = str(tmp_path / 'config.json')
    with open(cfg, 'w') as f:
        json.dump({'wavenet_config': wc.wavenet_config('small'), 'diffusion_config': synth.DIFFUSION_CONFIG}, f)
    den = create_diffwave_model(None, cfg, reverse_timestep=2, state_dict=wc.state_dict('small'), engine=small, any_length=True,
                                grad_backend='hip')
    x = (torch.from_numpy(np.stack([synth.synthetic_clip(i)[:, :1021] for i in (0, 5)])) * 0.8).cuda()       # [2, 1, 1021]
    grads = {}
    for backend in ('torch', 'hip'):
        den.model.grad_backend = backend
        den._draws = 0                                          # the same Philox keys on both branches
        xg = x.clone().requires_grad_(True)
        (g,) = torch.autograd.grad(den(xg).sum(), xg)
        grads[backend] = g.detach().cpu().numpy()
    err = wc.relmax(grads['hip'], grads['torch'])
    print('len 1021 through DiffWave.forward: hip vs torch gradient %.2e (bound 1e-3)' % err)
    assert grads['hip'].shape == (2, 1, 1021) and np.isfinite(grads['hip']).all() and np.abs(grads['hip']).max() > 0 and err <= 1e-3
    den._draws = 0
    out = den(x)
    den._draws = 0
    x_t = den._diffusion(x)
    den._draws = 0
    assert out.shape == x.shape and torch.equal(den._reverse(x_t), out)
    with pytest.raises(NotImplementedError, match='any_length=True'):
        den.one_shot_denoise(x)


# ---- 10. the driver ---------------------------------------------------------------------------------------------------------------------
def test_driver_native_length_diffusion(tmp_path):
    import kws_adaptive_attack_eval as drv
    from audio_models.RCNN_KWS.model import KWSModel
    from datasets.qualcomm_kws_dataset import CLASSES
    from diffusion_models.diffwave_ddpm import DiffWave, WaveNetHIP
    from oracle import dmad_oracle as orc
    root, rng = str(tmp_path / 'data'), np.random.RandomState(5)
    for i, (c, n) in enumerate(zip((0, 0, 1, 1, 2, 3), (4001, 8999, 6500, 4001, 8999, 6500))):
        os.makedirs(os.path.join(root, CLASSES[c]), exist_ok=True)
        mc.write_wav(os.path.join(root, CLASSES[c], 'clip_%02d.wav' % i), rng.uniform(-0.3, 0.3, n))
    args = drv.build_parser().parse_args(['--data_path', root, '--defense', 'Diffusion', '--attack', 'CW', '--max_iter_1', '2', '--t', '1',
                                          '--max_clip_len', '9088', '--verbose', '0'])
    eng = new_engine('small', clip_len=9088, max_batch=1)
    den = DiffWave(WaveNetHIP(eng, state_dict=wc.state_dict('small'), grad_backend='hip', any_length=True),
                   orc.calc_diffusion_hyperparams(**synth.DIFFUSION_CONFIG), reverse_timestep=1, noise_source='device', seed=SEED)
    net = KWSModel(in_size=32)
    net.load_state_dict(kc.state_dict())
    net.eval()
    seen = []                                                   # every no-grad call of the purifier: (keys before, input, output)
    den.register_forward_pre_hook(lambda m, a: seen.append([m._draws, a[0].detach().clone(), None]))
    den.register_forward_hook(lambda m, a, out: seen[-1].__setitem__(2, None if out.requires_grad else out.detach().clone()))
    out = drv.run(args, classifier=net, defender=den, engine=eng, log=lambda *a: None)
    assert out['total'] == 6 and all(np.isfinite(out[k]) and 0.0 <= out[k] <= 100.0 for k in ('clean_acc', 'denoised_acc', 'robust_acc'))
    system, _ = drv.build_system(args, net, den, eng)
    data = drv.build_dataset(args)
    assert sorted(len(data[i]['samples']) for i in range(6)) == [4001, 4001, 6500, 6500, 8999, 8999]
    hooked, correct = len(seen), 0
    for i in range(6):
        clip = torch.from_numpy(data[i]['samples']).view(1, 1, -1).cuda()
        draws, _, purified = next(s for s in seen[:hooked] if s[2] is not None and s[1].shape == clip.shape and torch.equal(s[1], clip))
        den._draws = draws
        with torch.no_grad():
            again = system.defender(clip)                       # the purifier called directly at this clip's length, with the run's keys
            assert torch.equal(again, purified), i
            correct += int(system(purified, False).argmax(1).item() == data[i]['target'])
    assert out['denoised_acc'] == correct / 6 * 100
    with pytest.raises(ValueError, match='--max_clip_len 9088'):
        system.defender(torch.zeros(1, 1, 9089, device='cuda'))
    eng.close()
