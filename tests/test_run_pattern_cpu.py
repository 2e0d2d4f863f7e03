"""The run pattern the host chooses for a persistent call (csrc/cc4_sched.h: run_config_for_call), checked on the CPU.

tests/cpp/run_pattern_check.cpp -- a stand-alone program with its own main, never loaded into Python -- is built with the host compiler and the address /
undefined-behaviour sanitizers and run as a child process: for every call length 1 .. 2000 the runs tile the call's steps exactly, calls below the
long-call threshold keep run_split's default field for field, long calls close with ONE run instead of single steps, and an explicit pattern
(CC4_PERSIST_RUNS) passes through unchanged."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _compiler():
    for cxx in (os.environ.get('CXX'), 'g++', 'c++', 'clang++'):
        if cxx and shutil.which(cxx):
            return shutil.which(cxx)
    return None


def test_run_pattern_under_sanitizers(tmp_path, capsys):
    cxx = _compiler()
    if cxx is None:
        pytest.skip('no host C++ compiler found (CXX, g++, c++, clang++): the stand-alone check cannot be built')
    exe = str(tmp_path / 'run_pattern_check')
    flags = ['-std=c++17', '-O1', '-g', '-fsanitize=address,undefined', '-fno-sanitize-recover=undefined']
    if 'clang' not in subprocess.run([cxx, '--version'], capture_output=True, text=True).stdout:
        flags += ['-static-libasan', '-static-libubsan']
    cc = subprocess.run([cxx] + flags + ['-o', exe, os.path.join(ROOT, 'tests', 'cpp', 'run_pattern_check.cpp')], capture_output=True, text=True)
    assert cc.returncode == 0, cc.stdout + cc.stderr
    run = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert run.returncode == 0, run.stdout[-4000:] + run.stderr[-8000:]
    assert ' 0 failures' in run.stdout and 'run_pattern_check:' in run.stdout, run.stdout
    with capsys.disabled():
        print(f'\n  {run.stdout.strip().splitlines()[-1]}', end='')
