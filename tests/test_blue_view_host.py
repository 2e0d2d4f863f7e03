"""CPU: blue's own knowledge on the host.  blue_view.from_row (cc4_blue_view_from_row: the kernel's definition compiled for the host) against
blue_view.from_true_state (the independent restatement from the true-state document) on rows the CPU oracle produces while it replays the golden
trajectories recorded from the reference with the event log on -- the random-blue and structured-blue ones included, so that Analyse, decoys,
Block / Allow and Restore occur --, with the leak rule on every row; and the same rows without a cold row and with the log off."""
import json

import numpy as np
import pytest

import blue_util as BU
import golden_util as G
from cage_challenge_4_amd import blue_view as BV
from oracle_binding import OracleVecEnv
from test_oracle_golden import replay

if not (hasattr(OracleVecEnv, 'get_state') and hasattr(OracleVecEnv, 'get_cold') and hasattr(OracleVecEnv, 'true_state_json')):
    pytest.skip('the oracle binding exposes neither rows nor true-state documents', allow_module_level=True)

DOC_WORDS = list(BV.DOC_WORDS)
HOT_COLUMNS = [0, 1, 7]           # what a view without a cold row still carries per host (column 7: the Analyse part)


def _check(env, steps, what, seen, log_on=True):
    row, cold, d = env.get_state(0), env.get_cold(0), json.loads(env.true_state_json(0))
    hosts, scal = BV.from_row(row, cold, steps)
    th, ts = BV.from_true_state(d)
    bad = np.argwhere(hosts != th)
    assert bad.size == 0, (what, [tuple(map(int, b)) + (int(hosts[tuple(b)]), int(th[tuple(b)])) for b in bad[:8]])
    assert np.array_equal(scal[:, DOC_WORDS], ts[:, DOC_WORDS]), (what, scal.tolist(), ts.tolist())
    h0, s0 = BV.from_row(row, cold, 0)                      # steps 0: the episode length the row records
    assert np.array_equal(h0, hosts) and np.array_equal(s0, scal), what
    # the leak rule: outside the hosts of the agent's zone nothing but column 5, and that only for this step's remote addresses
    zone, remote = BU.allowed_rows(d), BU.remote_rows(d)
    assert not hosts[~zone][:, [0, 1, 2, 3, 4, 6, 7]].any(), (what, 'a row outside the zone carries more than column 5')
    assert not hosts[~remote][:, 5].any() and (hosts[remote][:, 5] > 0).all(), (what, 'column 5 and the remote addresses of the step disagree')
    assert (hosts[zone][:, 0] == 1).all(), what
    valid = bool(scal[0, 10])
    assert (scal[:, 10] == int(valid)).all() and valid == (log_on and d['step'] >= 1), (what, scal[:, 10].tolist())
    idle = scal[:, 0] == 0
    assert (scal[idle, 1] == 0).all() and (scal[idle, 2] == 255).all() and (scal[idle, 3] == 0).all(), what
    assert (scal[~idle, 1] >= 2).all() and (scal[~idle, 3] >= 1).all() and (scal[~idle, 7] == BV.T_IN_PROGRESS).all(), what
    assert (scal[~idle, 4] == 0).all() and not hosts[~idle][..., 7].any() and (scal[:, 14:] == 0).all(), what
    assert np.array_equal(scal[:, 11], hosts[..., 3:5].astype(np.int64).sum(axis=(1, 2))) or (hosts[..., 3:5] == 255).any(), what
    # without the cold row: no event columns, no sus_pids, no decoy bits; everything that lives in the hot row is the same
    hn, sn = BV.from_row(row, None, steps)
    assert not hn[..., 2:7].any() and (sn[:, 10] == 0).all() and (sn[:, 11] == 0).all(), what
    analyse = scal[:, 4] == BV.ANALYSE
    assert np.array_equal(hn[..., [0, 1]], hosts[..., [0, 1]]) and np.array_equal(hn[analyse][..., 7], hosts[analyse][..., 7]) and not hn[~analyse][..., 7].any(), what
    keep = [k for k in range(16) if k not in (10, 11)]
    assert np.array_equal(sn[:, keep], scal[:, keep]), what
    if seen is not None:
        seen['col_max'] = np.maximum(seen['col_max'], hosts.reshape(-1, 8).max(axis=0))
        seen['word_max'] = np.maximum(seen['word_max'], scal.max(axis=0))
        seen['success'] |= set(scal[:, 7].tolist())
        seen['own'] |= set(np.unique(hosts[..., 7]).tolist())
        seen['outside'] += int(hosts[~zone][:, 5].astype(bool).sum())
        seen['n'] += 1
    return hosts, scal


def test_host_function_matches_the_document_over_the_golden_trajectories(oracle_lib):
    fixes = [G.load(p) for p in G.list_fixtures()]
    names = ' '.join(f['name'] for f in fixes)
    # the random-blue fixtures and the structured-blue ones (a fixed pattern of one action class each, and their mix)
    assert len(fixes) >= 30 and all(k in names for k in ('_random_', '_analyse_', '_decoy_', '_block_allow_', '_remove_', '_restore_', '_mix_')), names
    seen = dict(col_max=np.zeros(8, np.int64), word_max=np.zeros(16, np.int64), success=set(), own=set(), outside=0, n=0)
    for fix in fixes:
        env, _obs = replay(OracleVecEnv, fix, red_policy=fix['red_policy'], green_policy=fix['green_policy'], blue_policy=fix['blue_policy'])
        env.enable_event_log(True)
        _check(env, fix['steps'], (fix['name'], 'reset'), seen)
        T = min(fix['actions'].shape[0], 150)
        for t in range(T):
            env.step(fix['actions'][t][None], None if fix['messages'] is None else fix['messages'][t][None])
            if t % 10 == 9 or t == T - 1:
                _check(env, fix['steps'], (fix['name'], t), seen)
        env.close()
    assert seen['n'] > 400
    assert (seen['col_max'] > 0).all(), seen['col_max'].tolist()                                   # every column moved
    assert (seen['word_max'][:14] > 0).all() and (seen['word_max'][14:] == 0).all(), seen['word_max'].tolist()   # every word but the reserved ones
    assert seen['success'] >= {BV.T_TRUE, BV.T_UNKNOWN, BV.T_FALSE, BV.T_IN_PROGRESS}, seen['success']
    files = {o & 7 for o in seen['own'] if 0 < o < BV.OWN_DECOY}
    assert any(o & 1 for o in files) and any(o & 2 for o in files), seen['own']                    # Analyse found cmd.sh, and escalate.sh
    assert any(o & BV.OWN_DECOY for o in seen['own']) and seen['outside'] > 0, seen['own']         # a decoy; a remote host outside the zone
    assert seen['col_max'][3] >= 10 and seen['col_max'][2] >= 1, seen['col_max'].tolist()         # a brute force's ten entries; a suspicious pid


def test_log_off_keeps_the_hot_row_part_and_a_stale_log_is_not_reported(oracle_lib):
    fix = next(G.load(p) for p in G.list_fixtures() if 'random_ctor_500' in p)
    env, _obs = replay(OracleVecEnv, fix, red_policy=fix['red_policy'], green_policy=fix['green_policy'], blue_policy=fix['blue_policy'])
    env.enable_event_log(True)
    for t in range(30):
        env.step(fix['actions'][t][None])
    on_h, on_s = _check(env, fix['steps'], 'log on', None)
    assert on_s[0, 10] == 1 and on_h[..., 3:7].any()
    env.enable_event_log(False)                 # the log keeps the entries of step 29; the flag alone makes them invalid
    off_h, off_s = _check(env, fix['steps'], 'log switched off', None, log_on=False)
    assert not off_h[..., 3:7].any() and np.array_equal(off_h[..., :3], on_h[..., :3]) and (off_s[:, 11] == 0).all()
    env.enable_event_log(True)                  # switched on again without a step: still the entries of step 29 -- valid
    _check(env, fix['steps'], 'log on again', None)
    env.enable_event_log(False)
    for t in range(30, 40):
        env.step(fix['actions'][t][None])       # the log now describes step 29, the row step 40
    h1, s1 = _check(env, fix['steps'], 'log off', None, log_on=False)
    assert (s1[:, 10] == 0).all() and not h1[..., 3:7].any() and h1[..., 2].any() and s1[:, 8].sum() > 0
    row, cold = env.get_state(0), env.get_cold(0).copy()
    env.enable_event_log(True)                  # enabled, but its step stamp is 29 and the row has taken step 39: stale
    h2, s2 = _check(env, fix['steps'], 'stale', None, log_on=False)
    assert np.array_equal(h2, h1) and np.array_equal(s2, s1)
    env.close()
    with pytest.raises(ValueError):
        BV.from_row(row[:-1], cold)
    hb, sb = BV.from_row(bytes(row), bytes(cold), fix['steps'])         # any buffer, at any address
    assert hb.shape == (5, 137, 8) and hb.dtype == np.uint8 and sb.shape == (5, 16) and sb.dtype == np.int32
    assert np.array_equal(hb, h1) and np.array_equal(sb, s1)
