"""What the stand-alone C++ checks under tests/cpp share: find a host compiler, build one source file at -O1 with the address and undefined-behaviour
sanitizers, run the program as a child process (never loaded into Python), require exit status 0.  What the program printed is the caller's to judge."""
import os
import shutil
import subprocess
import time

import pytest

NO_COMPILER = 'no host C++ compiler found (CXX, g++, c++, clang++): the stand-alone check cannot be built'


def compiler():
    for cxx in (os.environ.get('CXX'), 'g++', 'c++', 'clang++'):
        if cxx and shutil.which(cxx):
            return shutil.which(cxx)
    return None


def build_and_run(src, tmp_path, required, timeout, flags=()):
    """The finished child process (exit status 0 asserted; .seconds: how long it ran).  required: without a compiler the test fails (the oracle needs one
    too) instead of skipping.  flags: the file's own beside -std=c++17 -O1 -g and the sanitizers (-ffp-contract=off where it compares floating point)."""
    cxx = compiler()
    if cxx is None:
        assert not required, NO_COMPILER + ' (the oracle needs one too)'
        pytest.skip(NO_COMPILER)
    exe = str(tmp_path / os.path.splitext(os.path.basename(src))[0])
    flags = ['-std=c++17', '-O1', '-g', *flags, '-fsanitize=address,undefined', '-fno-sanitize-recover=undefined']
    # the sanitizer runtimes inside the program itself (clang's default; gcc needs to be told), so that it depends on no shared runtime
    if 'clang' not in subprocess.run([cxx, '--version'], capture_output=True, text=True).stdout:
        flags += ['-static-libasan', '-static-libubsan']
    cc = subprocess.run([cxx] + flags + ['-o', exe, src], capture_output=True, text=True)
    assert cc.returncode == 0, cc.stdout + cc.stderr
    t0 = time.time()
    run = subprocess.run([exe], capture_output=True, text=True, timeout=timeout)
    run.seconds = time.time() - t0
    assert run.returncode == 0, run.stdout + run.stderr
    return run
