"""CPU: the word view of the red agents' header and of the action records (csrc/cc4_state.h: RedHdrW / ActW, hget / hset / hinc, aget / aset,
act_word / act_pack / act_unpack, act_tick, hdr_tick_reset, hdr_obs_word, hdr_load / hdr_store) against member loads and stores of RedHdr and
Act.  tests/cpp/hdr_words_check.cpp is a stand-alone program with its own main: built here with the host compiler at -O1 with the address and
undefined-behaviour sanitizers and run as a child process (never loaded into Python).  Over 20 000 random headers and records, for every
field: get == the member; set of 0, 1, the maximum, both sides of every byte boundary and values with bits above the field == the member
store with every other byte untouched; the increment wraps as the member does; the tick's masks == the five resets field by field;
obs_first as one word with obs_success set and not set; ticks-- on the word for ticks 1, 2, 0 and 255.  Exit status 0: all agreed."""
import os

from cpp_check import build_and_run


ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, 'tests', 'cpp', 'hdr_words_check.cpp')


def test_word_view_equals_member_access(tmp_path):
    run = build_and_run(SRC, tmp_path, required=True, timeout=300)
    assert ' 0 mismatches' in run.stdout, run.stdout
