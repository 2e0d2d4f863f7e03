"""CPU: the surface of the red agents as learners -- header, exports, bindings, constants, the kernels' resource rows (as committed in
profiles/kernel_resources.txt, which build() rewrites from the compiler's metadata of every build: the test shows that the file lists the two
kernels without scratch, not what a library built elsewhere holds) -- and the stand-alone
check of the shared record conversion (csrc/cc4_red_view.h: red_record, red_auto_sid) and of the host view on hand-made rows.
tests/cpp/red_record_check.cpp is a program with its own main: built here with the host compiler at -O1 with the address and
undefined-behaviour sanitizers and run as a child process (never loaded into Python).  It checks every refusal rule against the host loop of
cc4_step_ex over a grid of types, hosts and args, the record's bytes member by member, SID_AUTO with no, one and several sessions, and that a
row from elsewhere (list entries past the pool, hosts past the table, lengths past the lists) is never read past.  Exit status 0: all agreed."""
import os
import re

from conftest import ROOT
from cpp_check import build_and_run

SRC = os.path.join(ROOT, 'tests', 'cpp', 'red_record_check.cpp')


def test_surface_header_exports_bindings_constants_and_resources():
    import ctypes
    from cage_challenge_4_amd import _lib
    from cage_challenge_4_amd import red_view as RV
    txt = open(os.path.join(ROOT, 'include', 'cc4.h')).read()
    code = re.sub(r'/\*.*?\*/', '', txt, flags=re.S)
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for sym, nargs in (('cc4_step_red_device', 4), ('cc4_red_view_device', 7), ('cc4_red_view_from_row', 3), ('cc4_red_record_from_row', 4)):
        assert re.search(r'\bint\s+' + sym + r'\s*\(', code), sym
        assert hasattr(lib, sym), sym
        assert len(_lib.SIGNATURES[sym][1]) == nargs, sym
    assert f'#define CC4_RED_ACT_WORDS {RV.ACT_WORDS} ' in txt and RV.ACT_WORDS == len(RV.ACTION_WORDS) == 4
    assert re.search(r'#define CC4_RED_SID_AUTO\s+\(-1\)', txt) and RV.SID_AUTO == -1
    assert f'#define CC4_RED_VIEW_HOSTS {RV.VIEW_HOSTS}\n' in txt and RV.VIEW_HOSTS == 137
    assert f'#define CC4_RED_VIEW_PER_HOST {RV.VIEW_PER_HOST}\n' in txt and RV.VIEW_PER_HOST == 8
    assert f'#define CC4_RED_VIEW_SCALARS {RV.VIEW_SCALARS}\n' in txt and RV.VIEW_SCALARS == 16
    assert sorted(RV.HOST_COLUMNS.values()) == list(range(8)) and sorted(RV.SCALAR_WORDS.values()) == list(range(16))
    for name, c in RV.HOST_COLUMNS.items():          # the header's table names every column, in order
        assert re.search(rf'\*\s+{c} {name}\b', txt), name
    rows = {k: [ln for ln in open(os.path.join(ROOT, 'profiles', 'kernel_resources.txt')) if k in ln] for k in ('k_red_view', 'k_red_submit')}
    for k, r in rows.items():
        assert len(r) == 1 and r[0].rstrip().endswith('cc4_k_red.hip'), (k, r)
        assert re.search(r'scratch\s+0 vgpr_spill\s+0 sgpr_spill\s+0 ', r[0]), r[0]


def test_record_conversion_and_host_view_under_the_sanitizers(tmp_path):
    run = build_and_run(SRC, tmp_path, required=True, timeout=300, flags=['-ffp-contract=off'])
    assert ' 0 mismatches' in run.stdout, run.stdout
