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
BESIDE = ('selfcheck_all', 'selfcheck_last', 'selfcheck_pcg', 'selfcheck_random', 'neighbour_after', 'neighbour_before')     # the cells with something beside the kernel


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
    for cid in ('no_msgs', 'no_record', 'random_steps', 'steal_all', 'steal_late', 'pcg') + BESIDE:
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


def test_cells_beside_the_kernel_change_nothing_else():
    """A cell with something beside the kernel IS the cell it names, inputs and trajectory included (the oracle steps nothing new for it); check_premise
    keys on the cells' fields, so which ids carry which field values is pinned here."""
    twin = {'selfcheck_all': 'base', 'selfcheck_last': 'base', 'neighbour_after': 'base', 'neighbour_before': 'base', 'selfcheck_pcg': 'pcg',
            'selfcheck_random': 'random_steps'}
    assert set(twin) == set(BESIDE) == {c.id for c in H.CELLS.values() if c.beside is not None}
    for cid, of in twin.items():
        cell, plain = H.CELLS[cid], H.CELLS[of]
        assert cell._replace(id=of, beside=None, R=plain.R) == plain, cid
        assert H.oracle_trajectory(cell, N) is H.oracle_trajectory(plain, N), cid
        assert H.kernel_name(cell) == H.kernel_name(plain), cid
    assert {c.id for c in H.CELLS.values() if isinstance(c.call, H.Random)} == {'random_steps', 'selfcheck_random'}
    assert {c.id for c in H.CELLS.values() if c.rng_mode == 0} == {'pcg', 'selfcheck_pcg'}
    assert all((c.rng_mode, c.n) in ((1, 8192), (0, 6656)) for c in H.CELLS.values())
    on = H.SelfCheck('CC4_PERSIST_VERIFY', '1')
    assert [H.CELLS[c].beside for c in BESIDE] == [on, H.SelfCheck('CC4_PERSIST_VERIFY_EVERY', '4'), on, on, H.Neighbour('after'), H.Neighbour('before')]
    # selfcheck_last: a repetition is four persistent plan calls, so every fourth one is the 70-step call
    assert len(H.CELLS['selfcheck_last'].prefix) + 1 == 4 and H.CELLS['selfcheck_last'].call == H.CHILD_CALLS[3]
    # a premise that does not hold is caught from the fields, whatever the id
    traj = H.oracle_trajectory(H.CELLS['base'], N)
    for broken in (H.CELLS['selfcheck_last']._replace(beside=H.SelfCheck('CC4_PERSIST_VERIFY_EVERY', '3')), H.CELLS['base']._replace(n=6656),
                   H.CELLS['neighbour_after']._replace(beside=H.Neighbour('during')), H.CELLS['steal_all']._replace(beside=on),
                   H.CELLS['base']._replace(beside='shadow')):
        with pytest.raises(AssertionError):
            H.check_premise(broken, traj)
    with pytest.raises(AssertionError):
        H.check_premise(H.CELLS['pcg']._replace(call=H.Random(70)), H.oracle_trajectory(H.CELLS['pcg'], N))


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


def test_a_disagreement_under_the_self_check_names_the_side():
    """The verdict of a checked call with hand-made rows: main equal and shadow off; main off (shadow off too, shadow equal); return code 0 with main off."""
    cell = H.CELLS['selfcheck_all']
    traj = H.oracle_trajectory(cell, N)
    d = H.describe(cell, traj)
    said = ('CC4_PERSIST_VERIFY: k_run_philox1p and the per-step launches disagree after a plan of 70 steps: first episode 6 (hot row cold row outputs); first '
            'differing trajectory row: packed observations of step 69, 1 episode(s) differ in it, first episode 6')

    def final(hot=None, rng=None):
        return {'hot rows': (traj.hot if hot is None else hot, traj.hot), 'generator state': (traj.rng if rng is None else rng, traj.rng),
                'last observations': (traj.obs_last, traj.obs_last)}
    good = H.Side(traj.obs_packed, traj.rewards, traj.dones, final())
    hot = traj.hot.copy()
    hot[6, 40] ^= 8
    rng = traj.rng.copy()
    rng[6, 0] += 1
    shadow_off = H.Side(final=final(hot, rng))
    shadow_good = H.Side(final=final())
    # nothing to report: the call returned 0 and the main side is the oracle's
    assert H.self_check_verdict(cell, traj, 0, None, good) is None and H.self_check_verdict(cell, traj, 0, None, good, shadow_good) is None
    # main equal, shadow off: the shadow's episodes and partitions, the self-check's message in full
    msg = H.self_check_verdict(cell, traj, -5, said, good, shadow_off)
    assert msg.startswith('SHADOW LEFT THE TRAJECTORY') and 'KERNEL' not in msg and f'"{said}"' in msg, msg
    assert 'hot rows at the call\'s end differ in 1 episode(s), first [6] (partitions [6])' in msg and 'generator state' in msg and 'last observations' not in msg, msg
    # main off: the Location, and whether the shadow differs as well
    obs = traj.obs_packed.copy()
    obs[69, 6, 3] ^= 1
    off = H.Side(obs, traj.rewards, traj.dones, final(hot))
    want = H.Location(episode=6, step=69, run=len(d.runs) - 1, q=0, run_length=1, regeneration=False, partition=6)
    assert d.runs[-1] == (69, 1)
    for shadow, says in ((shadow_off, 'the shadow differs from the oracle too: hot rows'), (shadow_good, 'the shadow equals the oracle in everything fetched'),
                         (None, 'the shadow was not fetched')):
        msg = H.self_check_verdict(cell, traj, -5, said, off, shadow)
        assert msg.startswith('KERNEL LEFT THE TRAJECTORY') and 'SHADOW LEFT' not in msg and str(want) in msg and says in msg and f'"{said}"' in msg, msg
    # rc 0 with the main side off fails too: both sides wrong alike
    msg = H.self_check_verdict(cell, traj, 0, None, off, shadow_off)
    assert msg is not None and 'returned 0' in msg and 'both sides wrong alike' in msg and str(want) in msg and 'the shadow differs from the oracle too' in msg, msg
    # any other failure of the call is a failure, quoted
    assert 'rc=-1' in H.self_check_verdict(cell, traj, -1, 'hipErrorX', good) and 'hipErrorX' in H.self_check_verdict(cell, traj, -1, 'hipErrorX', good)
    # two handles beside each other: each against the same trajectory, the one that differs named
    ncell = H.CELLS['neighbour_after']
    assert H.neighbour_verdict(ncell, traj, (0, None, good), (0, None, good)) is None
    msg = H.neighbour_verdict(ncell, traj, (0, None, off), (0, None, good))
    assert 'A (the persistent kernel) LEFT THE TRAJECTORY' in msg and str(want) in msg and 'B (the per-step launches beside it) equals the oracle' in msg, msg
    msg = H.neighbour_verdict(ncell, traj, (0, None, good), (0, None, off))
    assert 'A (the persistent kernel) equals the oracle' in msg and 'B (the per-step launches beside it) LEFT THE TRAJECTORY' in msg, msg
    assert 'rc=-1' in H.neighbour_verdict(ncell, traj, (0, None, good), (-1, 'no memory', None))


def test_overlap_share_is_the_part_of_as_call_with_b_in_flight():
    assert H.overlap_share(0.0, 4.0, 1.0, 2.0) == 0.25 and H.overlap_share(1.0, 3.0, 0.0, 10.0) == 1.0        # B inside A; A inside B
    assert H.overlap_share(0.0, 2.0, 2.0, 5.0) == 0.0 and H.overlap_share(3.0, 5.0, 0.0, 2.5) == 0.0          # B wholly behind A; wholly in front (serialised)
    assert H.overlap_share(0.0, 4.0, 3.0, 9.0) == 0.25 and H.overlap_share(2.0, 6.0, 0.0, 3.0) == 0.25        # B starts late in A; B ends early in A
    assert H.overlap_share(1.0, 1.0, 0.0, 2.0) is None
