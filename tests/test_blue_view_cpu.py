"""CPU: the surface of blue's own knowledge -- header, exports, bindings, constants, the kernel's resource row (as committed in
profiles/kernel_resources.txt, which build() rewrites from the compiler's metadata of every build: the test shows that the file lists the kernel
without scratch, not what a library built elsewhere holds) -- and the stand-alone check of the serial statement (csrc/cc4_blue_view.h:
blue_view_from_row) on hand-made rows, logs and sus lists.
tests/cpp/blue_view_check.cpp is a program with its own main: built here with the host compiler at -O1 with the address and undefined-behaviour
sanitizers and run as a child process (never loaded into Python).  The log and the sus lists it hands over are heap blocks of exactly their size.
Exit status 0: all agreed."""
import os
import re

from conftest import ROOT
from cpp_check import build_and_run

SRC = os.path.join(ROOT, 'tests', 'cpp', 'blue_view_check.cpp')


def test_surface_header_exports_bindings_constants_and_resources():
    import ctypes
    from cage_challenge_4_amd import _lib
    from cage_challenge_4_amd import blue_view as BV
    txt = open(os.path.join(ROOT, 'include', 'cc4.h')).read()
    code = re.sub(r'/\*.*?\*/', '', txt, flags=re.S)
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for sym, nargs in (('cc4_blue_view_device', 7), ('cc4_blue_view_from_row', 5)):
        assert re.search(r'\bint\s+' + sym + r'\s*\(', code), sym
        assert hasattr(lib, sym), sym
        assert len(_lib.SIGNATURES[sym][1]) == nargs, sym
    assert f'#define CC4_BLUE_VIEW_HOSTS {BV.VIEW_HOSTS}\n' in txt and BV.VIEW_HOSTS == 137
    assert f'#define CC4_BLUE_VIEW_PER_HOST {BV.VIEW_PER_HOST}\n' in txt and BV.VIEW_PER_HOST == 8
    assert f'#define CC4_BLUE_VIEW_SCALARS {BV.VIEW_SCALARS}\n' in txt and BV.VIEW_SCALARS == 16
    assert f'#define CC4_BLUE_VIEW_PORT_PID 0x{BV.PORT_PID:02x}\n' in txt and f'#define CC4_BLUE_VIEW_OWN_DECOY 0x{BV.OWN_DECOY:02x}\n' in txt
    assert BV.NUM_BLUE == 5 and sorted(BV.HOST_COLUMNS.values()) == list(range(8)) and sorted(BV.SCALAR_WORDS.values()) == list(range(16))
    for name, c in BV.HOST_COLUMNS.items():          # the header's table names every column, in order
        assert re.search(rf'\*\s+{c} {name}\b', txt), name
    rows = [ln for ln in open(os.path.join(ROOT, 'profiles', 'kernel_resources.txt')) if 'k_blue_view' in ln]
    assert len(rows) == 1 and rows[0].rstrip().endswith('cc4_k_blue.hip'), rows
    assert re.search(r'scratch\s+0 vgpr_spill\s+0 sgpr_spill\s+0 ', rows[0]), rows[0]
    lds = int(re.search(r'lds_static\s+(\d+)', rows[0]).group(1))
    # two words per host, a half word per (agent, host), two words per agent: no more than four of LDS's 1280-byte granules, which is what 32
    # workgroups per CU -- a batch of 8192 on 256 CUs in one round -- leaves each
    assert 4 * (2 * 137 + (5 * 137 + 1) // 2 + 10) <= lds <= 4 * 1280, rows[0]


def test_serial_statement_on_crafted_rows_under_the_sanitizers(tmp_path):
    run = build_and_run(SRC, tmp_path, required=True, timeout=300, flags=['-ffp-contract=off'])
    assert ' 0 mismatches' in run.stdout, run.stdout
