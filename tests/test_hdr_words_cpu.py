"""CPU: the word view of the red agents' header and of the action records (csrc/cc4_state.h: RedHdrW / ActW, hget / hset / hinc, aget / aset,
act_word / act_pack / act_unpack, act_tick, hdr_tick_reset, hdr_obs_word, hdr_load / hdr_store) against member loads and stores of RedHdr and
Act.  tests/cpp/hdr_words_check.cpp is a stand-alone program with its own main: built here with the host compiler at -O1 with the address and
undefined-behaviour sanitizers and run as a child process (never loaded into Python).  Over 20 000 random headers and records, for every
field: get == the member; set of 0, 1, the maximum, both sides of every byte boundary and values with bits above the field == the member
store with every other byte untouched; the increment wraps as the member does; the tick's masks == the five resets field by field;
obs_first as one word with obs_success set and not set; ticks-- on the word for ticks 1, 2, 0 and 255.  Exit status 0: all agreed."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, 'tests', 'cpp', 'hdr_words_check.cpp')


def _compiler():
    for cxx in (os.environ.get('CXX'), 'g++', 'c++', 'clang++'):
        if cxx and shutil.which(cxx):
            return shutil.which(cxx)
    return None


def test_word_view_equals_member_access(tmp_path):
    cxx = _compiler()
    assert cxx is not None, 'no host C++ compiler found (CXX, g++, c++, clang++): the stand-alone check cannot be built (the oracle needs one too)'
    exe = str(tmp_path / 'hdr_words_check')
    flags = ['-std=c++17', '-O1', '-g', '-fsanitize=address,undefined', '-fno-sanitize-recover=undefined']
    # the sanitizer runtimes inside the program itself (clang's default; gcc needs to be told), so that it depends on no shared runtime
    if 'clang' not in subprocess.run([cxx, '--version'], capture_output=True, text=True).stdout:
        flags += ['-static-libasan', '-static-libubsan']
    cc = subprocess.run([cxx] + flags + ['-o', exe, SRC], capture_output=True, text=True)
    assert cc.returncode == 0, cc.stdout + cc.stderr
    run = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert run.returncode == 0, run.stdout + run.stderr
    assert ' 0 mismatches' in run.stdout, run.stdout
