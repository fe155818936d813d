"""The bookkeeping of the per-device kernel set-up (csrc/kernel_setup_table.h) on the host: tests/kernel_setup_table_main.cc is a
stand-alone program with counting stand-ins for the configure functions, built with the address and undefined-behaviour sanitizers
(host code only, its own main, so nothing is preloaded).  It asserts: a family is configured once per device; device 1 gets its own
configuration after device 0; a mask of several families configures each missing one once; a failing configure returns its error and is
tried again; eight threads asking for one pair at once run its function once.  Its exit status is the verdict."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, 'diffusion-model-for-audio-defense_amd', 'csrc')


def test_setup_table_under_sanitizers(tmp_path):
    exe = str(tmp_path / 'kernel_setup_table_main')
    subprocess.run(['g++', '-std=c++17', '-O1', '-g', '-Wall', '-Wextra', '-Werror', '-fsanitize=address,undefined', '-fno-sanitize-recover=all',
                    '-pthread', '-I', CSRC, os.path.join(ROOT, 'tests', 'kernel_setup_table_main.cc'), '-o', exe], check=True, timeout=120)
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=60)
    print(r.stdout)
    assert r.returncode == 0, r.stdout
    assert 'all checks passed' in r.stdout
