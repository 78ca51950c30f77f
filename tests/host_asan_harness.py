"""What the tests of the stand-alone sanitizer programs share: tests/host_asan/build_and_run.sh NAME builds
tests/host_asan/NAME.cpp against the library's host half and the HIP stand-in under AddressSanitizer +
UndefinedBehaviorSanitizer and runs it. Sanitizers run on these CPU programs only; nothing here is
loaded into Python."""
import os
import subprocess

from conftest import ROOT


def run_harness(name, tmp_path):
    """Builds and runs the program of `name` ('driver' or a family); asserts that it ended clean, with
    no sanitizer report and nothing left allocated. Returns its output and the output's lines."""
    prefix = 'host_asan' if name == 'driver' else 'host_asan_' + name
    script = os.path.join(ROOT, 'tests', 'host_asan', 'build_and_run.sh')
    proc = subprocess.run(['bash', script, name, str(tmp_path)], capture_output=True, text=True, timeout=900)
    out = proc.stdout + proc.stderr
    assert proc.returncode == 0, out[-4000:]
    assert '%s: ok' % prefix in out, out[-2000:]
    assert 'ERROR: AddressSanitizer' not in out and 'runtime error:' not in out and 'LeakSanitizer' not in out, out[-4000:]
    lines = out.splitlines()
    # nothing the library allocated outlives its handles
    report = [l for l in lines if l.startswith('hip_stub:') and 'live allocations' in l]
    assert report and report[-1].rstrip().endswith('live allocations 0'), report
    return out, lines


def launched(lines, kernel):
    """A `launches` line of the stand-in's report names this kernel."""
    return any(kernel in l for l in lines if l.strip().startswith('launches'))


def shape_only(lines, kernel):
    """The stand-in checked this kernel's launches for their shape alone: it has no shadow for it."""
    return any(kernel in l for l in lines if 'launch shape only' in l)
