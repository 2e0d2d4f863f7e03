"""CPU: the cells of the plan-kernel hand-over tests (tests/handover_util.py) still isolate what they claim to -- asserted with the oracle alone, at 8
episodes (a regeneration falls on the same step for every episode), so that an edited seed or length cannot quietly turn `regen_first` into another
`base`.  And the machinery the GPU module (tests/test_plan_handover.py) reports with: the packing of the oracle's observations, the place a step has in the
call's runs, the message of a mismatch."""
import ast
import re

import numpy as np
import pytest

import handover_util as H

N = 8


@pytest.mark.parametrize('cid', list(H.CELLS))
def test_cell_premise(cid):
    cell = H.CELLS[cid]
    traj = H.oracle_trajectory(cell, N)
    d = H.check_premise(cell, traj)
    # every step of the call is in exactly one run, at the position locate() gives it
    K = cell.call.k
    seen = []
    for j in range(K):
        loc = H.locate(cell, traj, j % N, j)
        assert d.runs[loc.run][0] + loc.q == j and 0 <= loc.q < loc.run_length == d.runs[loc.run][1], (j, loc)
        assert loc.regeneration == bool(traj.regen[j, j % N]) and loc.partition == (j % N) % H.PARTITIONS
        seen.append((loc.run, loc.q))
    assert len(set(seen)) == K
    assert traj.obs_packed.shape == (K, N, H.OBS_PACKED) and traj.rewards.shape == traj.dones.shape == traj.regen.shape == (K, N)
    assert np.array_equal(traj.obs[-1], traj.obs_last) and np.array_equal(traj.rewards[-1], traj.reward_last) and np.array_equal(traj.dones[-1], traj.done_last)


def test_single_factor_cells_keep_the_base_description():
    """The cells that change messages, recording, the generator, the entry point or the stealing threshold run the call cut as `base` cuts it, with the
    regenerations at the same places."""
    base = H.describe(H.CELLS['base'], H.oracle_trajectory(H.CELLS['base'], N))
    for cid in ('no_msgs', 'no_record', 'random_steps', 'steal_all', 'steal_late', 'pcg'):
        cell = H.CELLS[cid]
        assert H.describe(cell, H.oracle_trajectory(cell, N)) == base, cid
        assert [c.k for c in cell.prefix] == [c.k for c in H.CELLS['base'].prefix] and cell.call.k == H.CELLS['base'].call.k, cid
    for cid in ('no_regen', 'regen_first', 'regen_last'):
        cell = H.CELLS[cid]
        assert H.describe(cell, H.oracle_trajectory(cell, N)).runs == base.runs, cid
    assert dict(H.CELLS['steal_all'].knobs) == {'CC4_PERSIST_THR': '0'}
    assert all(not c.knobs for c in H.CELLS.values() if c.id not in ('steal_all', 'steal_late', 'every_step_a_run'))
    # steal_late: a wave leaves its partition only once that one is handed out -- the threshold is beyond the tickets a partition has in the call
    biggest = -(-H.CELLS['steal_late'].n // H.PARTITIONS) * len(base.runs)
    assert int(dict(H.CELLS['steal_late'].knobs)['CC4_PERSIST_THR']) > biggest


def test_base_is_the_self_check_childs_last_call():
    """`base` claims to be the failing call itself: the (k, rec, m) rows of test_plan's child script, its episode length and its seeds."""
    import test_plan
    src = test_plan._VERIFY_CHILD
    rows = ast.literal_eval(re.search(r'for k, rec, m in (\(\(.*?\)\)):', src).group(1))
    assert tuple(H.Plan(k, m, rec) for k, rec, m in rows) == H.CHILD_CALLS
    base = H.CELLS['base']
    assert base.prefix + (base.call,) == H.CHILD_CALLS and not base.knobs
    assert f'steps={base.steps},' in src and f'reset(seeds={H.RESET_SEED})' in src and 'default_rng(n)' in src and '(8192, 1), (6656, 0)' in src
    assert (H.CELLS['pcg'].n, H.CELLS['pcg'].rng_mode) == (6656, 0) and (base.n, base.rng_mode) == (8192, 1)


def test_packing_round_trips_and_matches_the_product():
    from cage_challenge_4_amd.vec_env import unpack_obs_rows
    rng = np.random.default_rng(3)
    obs = rng.integers(0, 4, size=(5, H.OBS)).astype(np.int32)
    p = H.pack_obs(obs)
    assert p.shape == (5, H.OBS_PACKED) and np.array_equal(H.unpack_obs(p), obs) and np.array_equal(unpack_obs_rows(p), obs)
    assert not (p[:, H.OBS // 4] >> (2 * (H.OBS % 4))).any() and not p[:, H.OBS // 4 + 1:].any()          # the bits past the last value are zero
    with pytest.raises(AssertionError):
        H.pack_obs(np.full((1, H.OBS), 4, np.int32))
    with pytest.raises(AssertionError):
        H.pack_obs(np.full((1, H.OBS), -1, np.int32))


def test_a_mismatch_is_reported_with_its_place_in_the_schedule():
    cell = H.CELLS['base']
    traj = H.oracle_trajectory(cell, N)
    d = H.describe(cell, traj)
    final = {'hot rows': (traj.hot, traj.hot), 'generator state': (traj.rng, traj.rng)}
    assert H.first_mismatch(cell, traj, traj.obs_packed, traj.rewards, traj.dones, final) is None
    assert H.first_mismatch(cell, traj, None, traj.rewards, None, None) is None
    j, run, q, ln = d.regens[0]
    obs = traj.obs_packed.copy()
    obs[j, 5, 17] ^= 4                       # one value of one episode, at a regeneration ..
    obs[j + 3, 2, 0] ^= 1                    # .. and a later difference that must not be the one reported
    rew = traj.rewards.copy()
    rew[j, 6] += 1.0
    hot = traj.hot.copy()
    hot[5, 100] ^= 1
    msg = H.first_mismatch(cell, traj, obs, rew, traj.dones, {'hot rows': (hot, traj.hot), 'generator state': (traj.rng, traj.rng)})
    want = H.Location(episode=5, step=j, run=run, q=q, run_length=ln, regeneration=True, partition=5)
    assert str(want) in msg and 'observations rewards' in msg and '2 episode(s) differ at that step' in msg, msg
    assert 'hot rows' in msg and 'first [5]' in msg and 'generator state' not in msg, msg
    # a step that is no regeneration; rewards compare as bit patterns
    rew = traj.rewards.copy()
    rew[j + 1, 3] = -rew[j + 1, 3] if rew[j + 1, 3] else -0.0
    msg = H.first_mismatch(cell, traj, None, rew, traj.dones)
    assert str(H.locate(cell, traj, 3, j + 1)) in msg and 'regeneration=False' in msg and '(rewards)' in msg, msg
