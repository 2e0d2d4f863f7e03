"""CPU: the scenario generation leaves the same bytes as before it was folded into one set of phase functions (csrc/cc4_engine.h env_reset).

tests/golden/reset_rows_parent.json holds, from the oracle of the commit that still had two generations, the zlib.crc32 of the hot row and of
the whole cold row of 128 seeds in every group of tools/record_reset_rows.py (RNG mode x episode length 30 / 500 / 1000 x default / non-default
policy word x, in counter mode, without / with a topology seed), after a fresh reset, after 12 steps and a continued reset, and after a second
continued reset.  This test recomputes all of them with the oracle of this tree and compares every entry; a mismatch names the group, the
stage and the seed."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tools'))
FIXTURE = os.path.join(ROOT, 'tests', 'golden', 'reset_rows_parent.json')


def test_reset_rows_equal_the_recorded_ones():
    import record_reset_rows as rec
    import oracle_binding
    oracle_binding.load()                                   # builds oracle/liboracle.so if it is missing
    want = json.load(open(FIXTURE))
    assert (want['seeds'], want['seed0'], want['steps_between'], want['stages']) == (rec.SEEDS, rec.SEED0, rec.STEPS_BETWEEN, list(rec.STAGES))
    names = [g[0] for g in rec.groups()]
    assert sorted(want['groups']) == sorted(names), 'the fixture and tools/record_reset_rows.py name different groups'
    got = rec.compute(oracle_binding.LIB)
    bad, compared = [], 0
    for name in names:
        for stage in rec.STAGES:
            w, g = want['groups'][name][stage], got[name][stage]
            assert len(w) == len(g) == rec.SEEDS
            for i in range(rec.SEEDS):
                compared += 1
                if w[i] != g[i]:
                    rows = ' and '.join(r for r, a, b in (('hot row', w[i][0], g[i][0]), ('cold row', w[i][1], g[i][1])) if a != b)
                    bad.append(f'{name} / {stage} / seed {rec.SEED0 + i}: {rows}')
    assert compared == len(names) * len(rec.STAGES) * rec.SEEDS == 18 * 3 * 128
    assert not bad, f'{len(bad)} of {compared} rows differ from the recorded ones, first: ' + '; '.join(bad[:8])
