"""CPU: the surface of the Monitor's connection edges -- header, exports, bindings, constants, the kernel's resource row (as committed in
profiles/kernel_resources.txt, which build() rewrites from the compiler's metadata of every build) -- and the stand-alone check of the serial
statement (csrc/cc4_blue_edges.h: blue_edges_from_row) against a std::map formulation on hand-made rows and logs.
tests/cpp/blue_edges_check.cpp is a program with its own main: built here with the host compiler at -O1 with the address and undefined-behaviour
sanitizers and run as a child process (never loaded into Python).  The row, the log and the outputs it hands over are heap blocks of exactly
their size.  Exit status 0: all agreed."""
import os
import re

from conftest import ROOT
from cpp_check import build_and_run

SRC = os.path.join(ROOT, 'tests', 'cpp', 'blue_edges_check.cpp')


def test_surface_header_exports_bindings_constants_and_resources():
    import ctypes
    from cage_challenge_4_amd import _lib
    from cage_challenge_4_amd import blue_edges as BE
    txt = open(os.path.join(ROOT, 'include', 'cc4.h')).read()
    code = re.sub(r'/\*.*?\*/', '', txt, flags=re.S)
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for sym, nargs in (('cc4_blue_edges_device', 8), ('cc4_blue_edges_from_row', 6)):
        assert re.search(r'\bint\s+' + sym + r'\s*\(', code), sym
        assert hasattr(lib, sym), sym
        assert len(_lib.SIGNATURES[sym][1]) == nargs, sym
    assert f'#define CC4_BLUE_EDGES_MAX {BE.MAX_EDGES}\n' in txt and BE.MAX_EDGES == 160 == BE.MAX_EVENTS
    assert f'#define CC4_BLUE_EDGES_COLUMNS {BE.EDGE_COLUMNS}\n' in txt and BE.EDGE_COLUMNS == 8
    assert f'#define CC4_BLUE_EDGES_WORDS {BE.EDGE_WORDS}\n' in txt and BE.EDGE_WORDS == 8
    assert (_lib.BLUE_EDGES_MAX, _lib.BLUE_EDGES_COLUMNS, _lib.BLUE_EDGES_WORDS) == (160, 8, 8)
    assert BE.NUM_BLUE == 5 and sorted(BE.COLUMNS.values()) == list(range(8)) and sorted(BE.WORDS.values()) == list(range(8))
    assert [BE.WORDS[k] for k in ('total', 'events_valid', 'step_count')] == [5, 6, 7]
    for name, c in BE.COLUMNS.items():          # the header's table names every column, in order
        assert re.search(rf'\*\s+{c} {name}\b', txt), name
    # the definition ties its constants to the log's capacity and to the header
    k_src = open(os.path.join(ROOT, 'cage_challenge_4_amd', 'csrc', 'cc4_k_edges.hip')).read()
    assert re.search(r'static_assert\(BE_MAX == CC4_BLUE_EDGES_MAX && BE_MAX == MAX_EV', k_src)
    rows = [ln for ln in open(os.path.join(ROOT, 'profiles', 'kernel_resources.txt')) if 'k_blue_edges' in ln]
    assert len(rows) == 1 and rows[0].rstrip().endswith('cc4_k_edges.hip'), rows
    assert re.search(r'scratch\s+0 vgpr_spill\s+0 sgpr_spill\s+0 ', rows[0]), rows[0]
    lds = int(re.search(r'lds_static\s+(\d+)', rows[0]).group(1))
    # 160 keys of 8 bytes and 160 rep words at the least; no more than four of LDS's 1280-byte granules, which is what 32 workgroups per CU -- a
    # batch of 8192 on 256 CUs in one round -- leaves each
    assert 160 * 12 <= lds <= 4 * 1280, rows[0]


def test_python_entry_points_check_max_edges():
    import numpy as np
    import pytest
    from cage_challenge_4_amd import _lib
    from cage_challenge_4_amd import blue_edges as BE
    hot = np.zeros(_lib.load().cc4_state_bytes(), np.uint8)
    for bad in (0, 161, -1):
        with pytest.raises(ValueError, match='max_edges'):
            BE.from_row(hot, None, 30, bad)
        with pytest.raises(ValueError, match='max_edges'):
            BE.from_true_state({'step': 0, 'hosts': []}, bad)
    edges, counts = BE.from_row(hot, None, 30, 3)                      # no cold row: no edges
    assert edges.shape == (3, 8) and (edges == -1).all() and not counts.any()
    edges, counts = BE.from_true_state({'step': 4, 'hosts': [], 'events': [], 'events_step': 2, 'events_total': 0}, 2)      # a stale log
    assert (edges == -1).all() and counts.tolist() == [0, 0, 0, 0, 0, 0, 0, 4]


def test_serial_statement_against_a_map_formulation_under_the_sanitizers(tmp_path):
    run = build_and_run(SRC, tmp_path, required=True, timeout=300, flags=['-ffp-contract=off'])
    assert ' 0 mismatches' in run.stdout, run.stdout
