"""CPU: the table form of the red FSM's option switch (csrc/cc4_engine.h: fsm_pk / fsm_pk_switch) and the per-lane forms
of the step's single-lane sections (rs_reserve_lane against rs_reserve, the pend_r ballot against step_red_merge, step_impact_term + step_end without
its loop against step_end).  tests/cpp/fsm_tail_forms_check.cpp is a stand-alone program with its own main: built here with the host compiler at -O1
with the address and undefined-behaviour sanitizers and run as a child process (never loaded into Python).  Exhaustive on the table (every state
0..255, both policies); the reservation over all 64 Exploit sets x pools whose next free records straddle every
word boundary, pools with 0..7 free records and random fills; the Impact sum over all phases x subnets x 64 sets.  Exit status 0: all agreed."""
import os

from cpp_check import build_and_run


ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, 'tests', 'cpp', 'fsm_tail_forms_check.cpp')


def test_fsm_tables_and_lane_forms_equal_their_serial_forms(tmp_path):
    run = build_and_run(SRC, tmp_path, required=False, timeout=300)
    assert ' 0 mismatches' in run.stdout, run.stdout
