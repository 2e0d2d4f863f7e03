"""CPU: the scenario generation (csrc/cc4_engine.h env_reset, both RNG modes, fresh and continued) and the four enumerations of the flat
observation (env_flat_obs, env_flat_obs_at, env_flat_obs_sorted, obs_fast_entry / obs_fast_value) on the host build of the engine, under the
address and undefined-behaviour sanitizers.  tests/cpp/reset_obs_check.cpp is a stand-alone program with its own main: built here with the
host compiler at -O1 and run as a child process (never loaded into Python).  It resets 64 seeds in each mode three times with 12 steps in
between, every row in a heap block of exactly its size, and compares the 578 values of every state across the four enumerations.  Exit
status 0: all agreed and the sanitizers found nothing."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, 'tests', 'cpp', 'reset_obs_check.cpp')


def _compiler():
    for cxx in (os.environ.get('CXX'), 'g++', 'c++', 'clang++'):
        if cxx and shutil.which(cxx):
            return shutil.which(cxx)
    return None


def test_generation_and_obs_enumerations_under_sanitizers(tmp_path):
    cxx = _compiler()
    if cxx is None:
        pytest.skip('no host C++ compiler found (CXX, g++, c++, clang++): the stand-alone check cannot be built')
    exe = str(tmp_path / 'reset_obs_check')
    flags = ['-std=c++17', '-O1', '-g', '-ffp-contract=off', '-fsanitize=address,undefined', '-fno-sanitize-recover=undefined']
    # the sanitizer runtimes inside the program itself (clang's default; gcc needs to be told), so that it depends on no shared runtime
    if 'clang' not in subprocess.run([cxx, '--version'], capture_output=True, text=True).stdout:
        flags += ['-static-libasan', '-static-libubsan']
    cc = subprocess.run([cxx] + flags + ['-o', exe, SRC], capture_output=True, text=True)
    assert cc.returncode == 0, cc.stdout + cc.stderr
    run = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert run.returncode == 0, run.stdout + run.stderr
    assert ' 384 generations' in run.stdout and ' 0 mismatches' in run.stdout, run.stdout
