"""Child process of test_gpu_kernel_setup.py (not a test module): a fresh process whose first calls into the library are the stateless op
exports whose launch needs the per-device dynamic-LDS attribute, before any engine exists.  Every result is measured against the
reference and the bound of that export's own op test (f32_ops_ref, unet16_ops_ref, wave_defense_cases; the f16 conv's 2e-3 / 2e-2 are
test_gpu_parity.test_gemm_h16_family_vs_torch_conv's) and printed in one JSON line as (error, bound, '<' or '<=' as that test compares);
the parent asserts.  dmad_wave_iir takes an engine for its clip length, so it runs after the others on an engine without WaveNet and
classifier, whose creation sets up the fp32 GEMM family alone.  With a second device visible the attention and the IIR export then run
there as well."""
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import f32_ops_ref as R  # noqa: E402
import unet16_ops_ref as U  # noqa: E402
import wave_defense_cases as wc  # noqa: E402  (puts the package on sys.path)

from dmad_hip import engine as E  # noqa: E402

ATT_CASE = (256, 1, 1, False)                                   # T = 256, the smallest head count and batch of R.ATT_CASES
H16_CASE = (2, 8, 64, 128, 9, 1, 0, False, 1, False)            # the smallest of test_gpu_parity.H16_CASES
X3_CASE = (7, 4, 256, 768, 1, 1, 0, 0, False, 1)                # ... of test_gpu_parity.X3_CASES
F32_CASE = (3, 8, 256, 10, 1, 1, 0, 0, False, 1)                # ... of R.CONV_CASES
IIR = 'order1'                                                  # the lowest order of wave_defense_cases.filters(), one clip


def attention(out):
    T, heads, B, _ = ATT_CASE
    qkv, go = R.att_inputs(ATT_CASE)
    o64, g64 = R.att_fwd_bwd(qkv, go, heads, torch.float64)
    out['attention_f32'] = (R.rel(E.qkv_attention_f32(qkv.cuda(), heads).cpu(), o64), R.F32_TOL, '<')
    gq = E.qkv_attention_bwd(qkv.cuda(), go.cuda(), heads)
    errs = [R.rel(a, r) for a, r in zip(R.split_qkv(gq.cpu(), heads), R.split_qkv(g64, heads))]
    out['attention_bwd'] = (max(errs), R.ATT_BWD_TOL, '<')
    q16 = qkv.half()
    err = (E.qkv_attention_h16(q16.cuda(), heads).cpu().double() - R.attention_ref(q16.double(), heads)).abs()
    out['attention_h16'] = (float((err / U.attention_h16_bound(q16, heads)).max()), 1.0, '<=')         # elementwise: err <= bound


def iir(out, eng):
    b, a = wc.filters()[IIR]
    x = wc.clips(11)[:1]
    y = eng.wave_iir(torch.from_numpy(x.copy()).cuda(), b, a)
    out['wave_iir'] = (float(np.abs(y.cpu().double().numpy() - wc.lfilter64(b, a, x)).max()), 8 * wc.iir_fp32_error(IIR, 'forward'), '<=')


def convs(out):
    B, H, cin, cout, taps, stride, _, _, _, _ = H16_CASE
    g = torch.Generator().manual_seed(1000 + B + H + cin)
    x = (torch.rand(B, H, H, cin, generator=g) * 2 - 1).half()
    w = ((torch.rand(1, taps, cout, cin, generator=g) * 2 - 1) * 0.1).half()
    bias = torch.rand(cout, generator=g) * 2 - 1
    o32, o16 = E.conv_h16(x.cuda(), w.cuda(), bias.cuda(), stride=stride)
    ref = R.conv_ref(x, w, None, bias, None, stride, False, dtype=torch.float32)
    out['conv_h16_fp32_out'] = (float((o32.cpu() - ref).abs().max()), 2e-3, '<')
    out['conv_h16_f16_out'] = (float((o16.cpu().float() - ref).abs().max()), 2e-2, '<')

    B, H, cin, cout, taps, stride, _, _, _, _ = X3_CASE
    g = torch.Generator().manual_seed(2000 + B + H + cin)
    x = torch.rand(B, H, H, cin, generator=g) * 2 - 1
    w = (torch.rand(1, taps, cout, cin, generator=g) * 2 - 1) * 0.1
    bias = torch.rand(cout, generator=g) * 2 - 1
    out['conv_x3'] = (R.rel(E.conv_x3(x.cuda(), w.cuda(), bias.cuda(), stride=stride).cpu(), R.conv_ref(x, w, None, bias, None, stride)), 1e-5, '<')

    B = F32_CASE[0]
    x, w, _, shift, _ = R.conv_inputs(F32_CASE, B)
    got, _ = E.conv_f32(x.cuda(), w.cuda(), shift.cuda())
    out['conv_f32'] = (R.rel(got.cpu(), R.conv_ref(x, w, None, shift)), R.F32_TOL, '<')
    g = torch.Generator().manual_seed(1)                        # test_conv_f32_reaches_every_dispatch_form's shape for the 8-slot narrow tile,
    x, w = torch.rand(1, 16, 16, 128, generator=g) * 2 - 1, (torch.rand(1, 9, 128, 128, generator=g) * 2 - 1) * 0.1      # the family's one kernel that needs the attribute
    got, choice = E.conv_f32(x.cuda(), w.cuda())
    out['conv_f32_narrow'] = (R.rel(got.cpu(), R.conv_ref(x, w)) if choice['narrow'] else float('inf'), R.F32_TOL, '<')


def main():
    report = {'devices': torch.cuda.device_count(), 'device0': {}, 'device1': {}}
    torch.cuda.set_device(0)
    attention(report['device0'])
    convs(report['device0'])
    eng = E.Engine(max_batch=8, precision=E.FP32, with_classifier=False, with_wavenet=False)
    iir(report['device0'], eng)
    eng.close()
    if report['devices'] >= 2:
        with torch.cuda.device(1):
            attention(report['device1'])
            eng = E.Engine(max_batch=8, precision=E.FP32, with_classifier=False, with_wavenet=False)
            iir(report['device1'], eng)
            eng.close()
    torch.cuda.synchronize()
    print('REPORT ' + json.dumps(report), flush=True)


if __name__ == '__main__':
    main()
