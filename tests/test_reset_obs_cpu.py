"""CPU: the scenario generation (csrc/cc4_engine.h env_reset, both RNG modes, fresh and continued) and the four enumerations of the flat
observation (env_flat_obs, env_flat_obs_at, env_flat_obs_sorted, obs_fast_entry / obs_fast_value) on the host build of the engine, under the
address and undefined-behaviour sanitizers.  tests/cpp/reset_obs_check.cpp is a stand-alone program with its own main: built here with the
host compiler at -O1 and run as a child process (never loaded into Python).  It resets 64 seeds in each mode three times with 12 steps in
between, every row in a heap block of exactly its size, and compares the 578 values of every state across the four enumerations.  Exit
status 0: all agreed and the sanitizers found nothing."""
import os

from cpp_check import build_and_run


ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, 'tests', 'cpp', 'reset_obs_check.cpp')


def test_generation_and_obs_enumerations_under_sanitizers(tmp_path):
    run = build_and_run(SRC, tmp_path, required=False, timeout=300, flags=['-ffp-contract=off'])
    assert ' 384 generations' in run.stdout and ' 0 mismatches' in run.stdout, run.stdout
