"""Record (or recompute) tests/golden/reset_rows_parent.json: checksums of the rows the CPU oracle's scenario generation leaves behind.

The fixture pins the generation (csrc/cc4_engine.h env_reset) byte for byte across a refactor: it is recorded once with the oracle built from the
commit the refactor starts from, and tests/test_reset_rows_cpu.py recomputes it with the oracle of the tree under test.

Groups: RNG mode (0 numpy stream, 1 counter) x episode length (30, 500, 1000) x policy word (0, and one non-default set) x, in counter mode only,
without / with a topology seed.  Per group 128 seeds; per seed the zlib.crc32 of the hot row (cc4o_state_ptr, cc4o_state_bytes) and of the whole
cold row at three stages: after a fresh cc4o_reset, after 12 oracle steps of random actions and a continued reset (continue_stream = 1), after a
second continued reset.

The cold row is summed as the recorded layout had it.  The fixed part has since grown by the reward record (EnvCold.rwd, between gfail and known_sid:
csrc/cc4_state.h); whatever the oracle's layout shows between the end of gfail and known_sid must be all zero after a regeneration -- which is the
record's own contract -- and is left out of the sum, so that every other byte of the row is still compared with the recording.  With an oracle of the
recorded layout the gap is empty and the sum is the whole row's.

  python tools/record_reset_rows.py [--lib oracle/liboracle.so] [--out tests/golden/reset_rows_parent.json]
"""
import argparse
import ctypes
import json
import os
import sys
import zlib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tests'))

SEEDS = 128
SEED0 = 7000
STEPS_BETWEEN = 12
STAGES = ('fresh', 'continued', 'continued_twice')
EPISODE_LENGTHS = (30, 500, 1000)
POLICY_SET = 1 | 0x10 | 0x20         # red policy 1, green policy 1, built-in blue policy (OracleVecEnv's policy word)
TOPOLOGY_SEED = 4242


def groups():
    """(name, rng_mode, steps, policy, topology_seed) of every recorded group."""
    out = []
    for mode in (0, 1):
        for steps in EPISODE_LENGTHS:
            for policy in (0, POLICY_SET):
                for topo in ((0,) if mode == 0 else (0, TOPOLOGY_SEED)):
                    name = f"{'numpy' if mode == 0 else 'counter'}-steps{steps}-policy{policy}" + ('-topo' if topo else '')
                    out.append((name, mode, steps, policy, topo))
    return out


def _bind(path):
    lib = ctypes.CDLL(path)
    vp, ci = ctypes.c_void_p, ctypes.c_int
    lib.cc4o_create2.restype = vp
    lib.cc4o_create2.argtypes = [ci, ci]
    lib.cc4o_destroy.argtypes = [vp]
    lib.cc4o_set_topology_seed.argtypes = [vp, ctypes.c_uint32]
    lib.cc4o_reset.argtypes = [vp, ci, ctypes.c_uint64, ci, ci, ci, ci]
    lib.cc4o_step.argtypes = [vp, ci, vp, vp]
    lib.cc4o_state_bytes.restype = ctypes.c_size_t
    lib.cc4o_state_ptr.restype = vp
    lib.cc4o_state_ptr.argtypes = [vp, ci]
    lib.cc4o_cold_bytes.restype = ctypes.c_size_t
    lib.cc4o_cold_bytes.argtypes = [vp]
    lib.cc4o_cold_ptr.restype = vp
    lib.cc4o_cold_ptr.argtypes = [vp, ci]
    lib.cc4o_layout.argtypes = [ctypes.c_char_p, ci]
    return lib


GFAIL_BYTES = 16                     # uint32_t gfail[4]


def _gap(lib):
    """[a, b): the bytes of the fixed part of the cold row between the end of gfail and known_sid (none in the recorded layout)."""
    buf = ctypes.create_string_buffer(8192)
    n = lib.cc4o_layout(buf, 8192)
    lay = {k: int(v) for k, v in (ln.split() for ln in buf.raw[:n].decode().splitlines())}
    a, b = lay['cold.gfail'] + GFAIL_BYTES, lay['cold.known_sid']
    assert 0 <= b - a <= 64 and (b - a) % 16 == 0, (a, b)
    return a, b


def compute(lib_path):
    """{group name: {stage: [[crc32 hot row, crc32 cold row] per seed]}} with the oracle library at lib_path."""
    import numpy as np
    from oracle_binding import random_actions
    lib = _bind(lib_path)
    nh = lib.cc4o_state_bytes()
    ga, gb = _gap(lib)
    out = {}
    for name, mode, steps, policy, topo in groups():
        h = ctypes.c_void_p(lib.cc4o_create2(SEEDS, steps))
        lib.cc4o_set_topology_seed(h, topo)
        nc = lib.cc4o_cold_bytes(h)

        def cold_crc(i):
            c = ctypes.string_at(lib.cc4o_cold_ptr(h, i), nc)
            if any(c[ga:gb]):
                raise AssertionError(f'{name}, seed {SEED0 + i}: bytes {ga}..{gb} of the cold row (behind gfail) are not zero after a regeneration')
            return zlib.crc32(c[:ga] + c[gb:])

        def crcs():
            return [[zlib.crc32(ctypes.string_at(lib.cc4o_state_ptr(h, i), nh)), cold_crc(i)] for i in range(SEEDS)]
        rec = {}
        for i in range(SEEDS):
            lib.cc4o_reset(h, i, SEED0 + i, mode, steps, 0, policy)
        rec[STAGES[0]] = crcs()
        for t in range(STEPS_BETWEEN):
            a = np.ascontiguousarray(random_actions(SEED0, t, SEEDS), np.int32)
            for i in range(SEEDS):
                lib.cc4o_step(h, i, a[i].ctypes.data_as(ctypes.c_void_p), None)
        for stage in STAGES[1:]:
            for i in range(SEEDS):
                lib.cc4o_reset(h, i, 0, mode, steps, 1, policy)
            rec[stage] = crcs()
        lib.cc4o_destroy(h)
        out[name] = rec
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('--lib', default=os.path.join(ROOT, 'oracle', 'liboracle.so'))
    ap.add_argument('--out', default=os.path.join(ROOT, 'tests', 'golden', 'reset_rows_parent.json'))
    args = ap.parse_args()
    doc = {'seeds': SEEDS, 'seed0': SEED0, 'steps_between': STEPS_BETWEEN, 'stages': list(STAGES), 'groups': compute(args.lib)}
    with open(args.out, 'w') as f:
        json.dump(doc, f, separators=(',', ':'))
        f.write('\n')
    print(f"{args.out}: {len(doc['groups'])} groups x {SEEDS} seeds x {len(STAGES)} stages, {os.path.getsize(args.out)} bytes")


if __name__ == '__main__':
    main()
