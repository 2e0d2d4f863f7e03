"""CPU: the red agents' view on the host.  red_view.from_row (cc4_red_view_from_row: the kernel's definition compiled for the host) against
red_view.from_true_state (the independent restatement from the true-state document) on rows the CPU oracle produces while it replays the
golden trajectories recorded from the reference -- every red class, both ways of starting an episode --, with the leak rule on every row; and
the record cc4_step_red_device makes of four words (cc4_red_record_from_row) on the same rows."""
import json

import numpy as np
import pytest

import golden_util as G
import red_util as RU
from cage_challenge_4_amd import red_view as RV
from oracle_binding import OracleVecEnv
from test_oracle_golden import replay

if not (hasattr(OracleVecEnv, 'get_state') and hasattr(OracleVecEnv, 'true_state_json')):
    pytest.skip('the oracle binding exposes neither rows nor true-state documents', allow_module_level=True)

DOC_WORDS = list(RV.DOC_WORDS)


def _check(env, what, seen):
    row, d = env.get_state(0), json.loads(env.true_state_json(0))
    hosts, scal = RV.from_row(row)
    th, ts = RV.from_true_state(d)
    bad = np.argwhere(hosts != th)
    assert bad.size == 0, (what, [tuple(map(int, b)) + (int(hosts[tuple(b)]), int(th[tuple(b)])) for b in bad[:8]])
    assert np.array_equal(scal[:, DOC_WORDS], ts[:, DOC_WORDS]), (what, scal.tolist(), ts.tolist())
    assert not hosts[~RU.allowed_rows(d)].any(), (what, 'a row of a host the agent knows nothing of is not zero')
    idle = scal[:, 1] == 0
    assert (scal[idle, 2] == 11).all() and (scal[idle, 3] == 255).all() and (scal[idle, 4] == 0).all(), what
    assert (scal[~idle, 2] <= 10).all() and (hosts[..., 7] == 0).all(), what
    for r in range(6):              # SID_AUTO in a record is the view's word 12 (0 where the agent has no session)
        rec, refused = RV.record_from_row(row, r, (9, 0, 0, RV.SID_AUTO))
        assert not refused and rec['type'][0] == 9 and rec['session'][0] == RV.auto_sid(d, r) == (0 if scal[r, 12] == RV.SID_NONE else scal[r, 12]), (what, r)
    seen['col_max'] = np.maximum(seen['col_max'], hosts.reshape(-1, 8).max(axis=0))
    seen['word_max'] = np.maximum(seen['word_max'], scal.max(axis=0))
    seen['levels'] |= set(np.unique(hosts[..., 2]).tolist())
    seen['inactive'] += int((scal[:, 0] == 0).sum())
    seen['n'] += 1


def test_host_function_matches_the_document_over_the_golden_trajectories(oracle_lib):
    fixes = [G.load(p) for p in G.list_fixtures()]
    assert len(fixes) >= 30 and {f['red_policy'] for f in fixes} == {0, 1, 2, 3}
    seen = dict(col_max=np.zeros(8, np.int64), word_max=np.zeros(16, np.int64), levels=set(), inactive=0, n=0)
    for fix in fixes:
        env, _obs = replay(OracleVecEnv, fix, red_policy=fix['red_policy'], green_policy=fix['green_policy'], blue_policy=fix['blue_policy'])
        _check(env, (fix['name'], 'reset'), seen)
        T = min(fix['actions'].shape[0], 150)
        for t in range(T):
            env.step(fix['actions'][t][None], None if fix['messages'] is None else fix['messages'][t][None])
            if t % 10 == 9 or t == T - 1:
                _check(env, (fix['name'], t), seen)
        env.close()
    assert seen['n'] > 400
    assert (seen['col_max'][:7] > 0).all() and seen['col_max'][7] == 0, seen['col_max'].tolist()       # every column moved; the reserved one never
    assert {0, 1, 2} <= seen['levels'] and seen['inactive'] > 0
    assert (seen['word_max'][[0, 1, 2, 4, 5, 9, 10, 12, 15]] > 0).all(), seen['word_max'].tolist()
    assert seen['col_max'][3] >= 2 and seen['word_max'][9] >= 4


def test_from_row_and_record_reject_other_sizes_and_refuse_out_of_range_words(oracle_lib):
    ora = OracleVecEnv(1, steps=30)
    ora.reset(seeds=3)
    row = ora.get_state(0)
    hosts, scal = RV.from_row(row)
    assert hosts.shape == (6, 137, 8) and hosts.dtype == np.uint8 and scal.shape == (6, 16) and scal.dtype == np.int32
    h2, s2 = RV.from_row(bytes(row))                # any buffer of the right size, at any address
    assert np.array_equal(hosts, h2) and np.array_equal(scal, s2)
    with pytest.raises(ValueError):
        RV.from_row(row[:-1])
    with pytest.raises(ValueError):
        RV.record_from_row(row, 0, (1, 2, 3))
    for words in ((11, 5, 0, 0), (4, 137, 0, -1), (0, 0, 9, -1), (8, 3, 200, 1), (-2, 0, 0, 0), (4, 3, 0, -2), (4, 3, 0, 65536)):
        rec, refused = RV.record_from_row(row, 0, words)
        assert refused and rec['type'][0] == -1, words
    rec, refused = RV.record_from_row(row, 0, (8, 3, 136, 17))
    assert not refused and (rec['type'][0], rec['host'][0], rec['arg'][0], rec['ticks'][0], rec['session'][0], rec['flags'][0]) == (8, 3, 136, 0, 17, 0)
    assert rec['rate0'][0] == 0.0 and rec['rate1'][0] == 0.0
    rec, refused = RV.record_from_row(row, 0, (-1, 999, 999, 999))
    assert not refused and rec['type'][0] == -1
    ora.close()
