"""CPU: who frees what a handle allocates.
1. csrc/cc4_owned.h, the list of (owning field, kind), with recording releasers in place of the runtime's: tests/cpp/owned_check.cpp is a stand-alone
   program with its own main, built with the host compiler at -O1 with the address and undefined-behaviour sanitizers and run as a child process
   (never loaded into Python).  Registration is idempotent per field and array elements are fields; releasing one field calls its kind's releaser
   once with the old value, nulls the field and keeps the entry; releasing everything takes each non-null field once, last registered first, and
   a second time calls nothing.  Exit status 0: all as expected.
2. The source: the host units allocate and free through the owner only (cc4_host.h: dev_alloc, pin_alloc, new_event, new_stream, release, DevTemp),
   and the main stream -> group streams event is recorded in one function (fork_groups)."""
import glob
import os
import re

from conftest import ROOT
from cpp_check import build_and_run

CSRC = os.path.join(ROOT, 'cage_challenge_4_amd', 'csrc')
RAW = ('hipMalloc(', 'hipHostMalloc(', 'hipFree(', 'hipHostFree(', 'hipEventCreate', 'hipEventDestroy', 'hipStreamCreate', 'hipStreamDestroy')


def test_the_list_under_the_sanitizers(tmp_path):
    run = build_and_run(os.path.join(ROOT, 'tests', 'cpp', 'owned_check.cpp'), tmp_path, required=True, timeout=120)
    assert 'owned_check: 0 failures' in run.stdout, run.stdout


def test_host_units_allocate_and_free_through_the_owner_only():
    units = sorted(glob.glob(os.path.join(CSRC, 'cc4_api*.hip')))
    assert len(units) >= 6
    found = [(os.path.basename(u), i + 1, ln.strip()[:100]) for u in units for i, ln in enumerate(open(u)) for raw in RAW if raw in ln]
    assert not found, found
    host = open(os.path.join(CSRC, 'cc4_host.h')).read()
    assert all(raw in host for raw in RAW), [raw for raw in RAW if raw not in host]
    assert 'hip' not in re.sub(r'//[^\n]*', '', open(os.path.join(CSRC, 'cc4_owned.h')).read()), 'cc4_owned.h knows no runtime'


def test_the_fork_event_is_recorded_in_one_function():
    recorded = []
    for u in sorted(glob.glob(os.path.join(CSRC, 'cc4_api*.hip'))):
        fn = None
        for ln in open(u):
            m = re.match(r'(?:static )?(?:[\w:<>]+[ *&]+)+(\w+)\([^;]*\)\s*\{\s*$', ln)      # a function's first line starts in column 0
            if m:
                fn = m.group(1)
            if re.search(r'hipEventRecord\(\s*h->mev\b', ln):
                recorded.append((os.path.basename(u), fn))
    assert recorded == [('cc4_api.hip', 'fork_groups')], recorded
