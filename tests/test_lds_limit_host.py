"""The bookkeeping of dl_lds_limit (csrc/error.cpp): the dynamic-LDS grant every kernel above 64 KiB needs, remembered per (device, kernel).
csrc/lds_limit_check.cpp compiles error.cpp into a host program with stand-ins for the two runtime calls and runs the cases below; the same
program runs again with the address / undefined-behaviour sanitizers and with the thread sanitizer in its HOST code.  Two devices in one process
have no GPU test: this is the evidence for that case."""
import os
import shutil
import subprocess

import pytest

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'deepliif_amd', 'csrc')
HIPCC = shutil.which('hipcc') or '/opt/rocm/bin/hipcc'
CASES = ['asks_once', 'second_device_asks_again', 'larger_asks_smaller_does_not', 'refusal_is_reported_and_retried', 'refused_increase_keeps_the_grant',
         '200_kernels_stay_remembered', 'eight_threads_ask_eight_times']
BUILDS = {
    'plain': [],
    'asan_ubsan': ['-Xarch_host', '-fsanitize=address,undefined', '-Xarch_host', '-fno-sanitize-recover=all'],
    'tsan': ['-Xarch_host', '-fsanitize=thread'],
}
_RUNS = {}


def _run(tmp_path_factory, build):
    """build and run the program once per build; -> the lines it printed"""
    if build in _RUNS:
        return _RUNS[build]
    if not os.path.exists(HIPCC):
        pytest.skip('hipcc not found')
    exe = str(tmp_path_factory.mktemp('lds_limit_' + build) / 'lds_limit_check')
    r = subprocess.run([HIPCC, '--cuda-host-only', '-O1', '-g', '-std=c++17', '-pthread', *BUILDS[build], '-x', 'hip', os.path.join(CSRC, 'lds_limit_check.cpp'),
                        '-o', exe], capture_output=True, text=True)
    if r.returncode != 0:
        # only a missing sanitizer RUNTIME is a reason to skip: the linker cannot find libclang_rt.*; anything else is a failure
        missing = [ln for ln in r.stderr.splitlines() if 'clang_rt' in ln and any(w in ln for w in ('cannot find', 'no such file', 'No such file', 'unable to find'))]
        if build != 'plain' and missing:
            pytest.skip('this toolchain cannot link the sanitizer runtime into a host program: ' + missing[0][:200])
        pytest.fail(f'lds_limit_check.cpp does not build ({build}):\n' + r.stderr[-3000:])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    _RUNS[build] = (r.returncode, r.stdout.splitlines(), r.stderr)
    return _RUNS[build]


@pytest.mark.parametrize('case', CASES)
def test_grant_bookkeeping(tmp_path_factory, case):
    code, lines, err = _run(tmp_path_factory, 'plain')
    assert f'ok {case}' in lines, (code, [ln for ln in lines if case in ln], err[-2000:])


@pytest.mark.parametrize('build', ['asan_ubsan', 'tsan'])
def test_grant_bookkeeping_under_sanitizers(tmp_path_factory, build):
    code, lines, err = _run(tmp_path_factory, build)
    assert code == 0 and lines == [f'ok {c}' for c in CASES], (code, lines, err[-3000:])
