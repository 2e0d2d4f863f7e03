"""CPU: the word-parallel forms of the green helpers and the wave-wide red zone check (csrc/cc4_engine.h: green_as_totals, green_lw_status,
green_as_dest, green_lw_active, nth_bit8, red_zone_table / red_foreign_lane / red_foreign_fold) against the loops they replace, which the
header keeps as *_loop functions.  tests/cpp/word_parallel_check.cpp is a stand-alone program with its own main: built here with the host
compiler at -O1 with the address and undefined-behaviour sanitizers and run as a child process (never loaded into Python).  It is
exhaustive where the domain is small (all 7-bit status patterns, all masks 1..255 x n below the population count, every nsvc, all 256
allowed masks x 2048 server-count words x every c below the total) and random on the live-host words.  Exit status 0: all agreed."""
import os

from cpp_check import build_and_run


ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, 'tests', 'cpp', 'word_parallel_check.cpp')


def test_word_parallel_forms_equal_their_loops(tmp_path):
    run = build_and_run(SRC, tmp_path, required=False, timeout=300)
    assert ' 0 mismatches' in run.stdout, run.stdout
