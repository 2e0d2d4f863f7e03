"""The run pattern the host chooses for a persistent call (csrc/cc4_sched.h: run_config_for_call), checked on the CPU.

tests/cpp/run_pattern_check.cpp -- a stand-alone program with its own main, never loaded into Python -- is built with the host compiler and the address /
undefined-behaviour sanitizers and run as a child process: for every call length 1 .. 2000 the runs tile the call's steps exactly, calls below the
long-call threshold keep run_split's default field for field, long calls close with ONE run instead of single steps, and an explicit pattern
(CC4_PERSIST_RUNS) passes through unchanged."""
import os

from cpp_check import build_and_run


ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_run_pattern_under_sanitizers(tmp_path, capsys):
    run = build_and_run(os.path.join(ROOT, 'tests', 'cpp', 'run_pattern_check.cpp'), tmp_path, required=False, timeout=300)
    assert ' 0 failures' in run.stdout and 'run_pattern_check:' in run.stdout, run.stdout
    with capsys.disabled():
        print(f'\n  {run.stdout.strip().splitlines()[-1]}', end='')
