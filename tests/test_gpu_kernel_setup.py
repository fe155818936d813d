"""Per-device kernel set-up on first use (csrc/kernel_setup.hip): one fresh child process (tests/kernel_setup_first_use.py) whose first
calls into the library are the stateless op exports that need the dynamic-LDS attribute, with no engine created before them, so the
lazy set-up depends neither on the order of the tests nor on dmad_create.  The child measures every result against the reference and the
bound of that export's own op test; the assertions are here.  With two devices visible the same child then runs the T = 256 attention and
the IIR export on device 1, which a per-process "once" would leave without the attribute."""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
DEVICE0 = ('attention_f32', 'attention_bwd', 'attention_h16', 'conv_h16_fp32_out', 'conv_h16_f16_out', 'conv_x3', 'conv_f32', 'conv_f32_narrow',
           'wave_iir')
DEVICE1 = ('attention_f32', 'attention_bwd', 'attention_h16', 'wave_iir')


@pytest.fixture(scope='module')
def report():
    r = subprocess.run([sys.executable, os.path.join(HERE, 'kernel_setup_first_use.py')], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True,
                       timeout=240)
    print(r.stdout[-4000:])
    assert r.returncode == 0, r.stdout[-4000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith('REPORT ')]
    assert len(lines) == 1, r.stdout[-4000:]
    return json.loads(lines[0][len('REPORT '):])


def _check(results, names):
    assert sorted(results) == sorted(names), sorted(results)
    for name in names:
        err, bound, cmp = results[name]
        print('%s: %.3e %s %.3e' % (name, err, cmp, bound))
        assert (err < bound) if cmp == '<' else (err <= bound), (name, err, cmp, bound)


def test_first_use_without_an_engine(report):
    _check(report['device0'], DEVICE0)


def test_second_device(report):
    if report['devices'] < 2:
        pytest.skip('one device visible')
    _check(report['device1'], DEVICE1)
