"""CPU: per-episode opponent classes (include/cc4.h "Mixed opponents in one batch") through the oracle, which compiles the engine's own regeneration.
The oracle is driven episode by episode with the DEFAULT policy argument; the classes are assigned in its rows with cc4_row_set_policies, the
host function of libcc4.so that states the same rule as the device kernels.
1. reference-anchored: every recorded trajectory of every class combination replays from an assignment alone;
2. the rule: an assignment takes effect at the next regeneration, never mid-episode, and CC4_POLICY_DEFAULT gives the argument's classes back;
3. cc4_row_set_policies / cc4_row_get_policies on single rows."""
import ctypes

import numpy as np
import pytest

import golden_util as G
import mix_util as M
from oracle_binding import OracleVecEnv
from plan_util import random_plan


# ---------------------------------------------------------------------------------------------------------------- 1. reference-anchored
def test_assigned_classes_replay_every_reference_trajectory(oracle_lib):
    """All traj_* fixtures -- redsleep, reddiscovery, redrandom, greensleep, the built-in blue among them --, one oracle per episode length, every
    cc4o_reset with policy argument 0 and the fixture's classes assigned in the row beforehand; seeded as test_oracle_golden.py seeds them (the ctor
    fixtures' second reset(None) is itself a regeneration under the assignment).  Observations, rewards, dones, masks and the PCG64 position after
    every step equal the recorded arrays."""
    allf = [G.load(p) for p in G.list_fixtures()]
    combos = {(f['red_policy'], f['green_policy'], f['blue_policy']) for f in allf}
    assert {c[0] for c in combos} == {0, 1, 2, 3} and {c[1] for c in combos} == {0, 1} and {c[2] for c in combos} == {0, 1}, combos
    for steps in sorted({f['steps'] for f in allf}):
        fixes = [f for f in allf if f['steps'] == steps]
        env = OracleVecEnv(len(fixes), steps=steps)
        assert env.policy == 0
        for i, f in enumerate(fixes):
            M.oracle_assign(env, i, f['red_policy'], f['green_policy'], f['blue_policy'])
            env.lib.cc4o_reset(env._h, i, ctypes.c_uint64(f['seed']), 0, steps, 0, 0)
            if f['reset_seed'] < 0:          # CybORG(seed=s); wrapper.reset()
                env.lib.cc4o_reset(env._h, i, 0, 0, steps, 1, 0)
            else:                            # wrapper.reset(seed=s+1)
                env.lib.cc4o_reset(env._h, i, ctypes.c_uint64(f['reset_seed']), 0, steps, 0, 0)
            env._collect(i, reward=False)
            live, assigned = M.row_get(M.oracle_row(env, i))
            assert live == assigned == (f['red_policy'], f['green_policy'], f['blue_policy']), f['name']
            assert np.array_equal(env._obs[i], f['obs'][0]), f['name']
        masks, rng = env.mask(), env.rng_state()
        for i, f in enumerate(fixes):
            assert np.array_equal(masks[i], f['mask']) and G.rng_words_match(f['rng'][0], rng[i]), f['name']
            for t in range(f['actions'].shape[0]):
                a = np.ascontiguousarray(f['actions'][t], np.int32)
                m = None if f['messages'] is None else np.ascontiguousarray(f['messages'][t], np.uint8)
                env.lib.cc4o_step(env._h, i, a.ctypes.data_as(ctypes.c_void_p), None if m is None else m.ctypes.data_as(ctypes.c_void_p))
                env._collect(i)
                assert np.array_equal(env._obs[i], f['obs'][t + 1]), (f['name'], t)
                assert env._rew[i] == f['reward'][t] and bool(env._done[i]) == bool(f['done'][t]) and env._err[i] == 0, (f['name'], t)
                w = np.zeros(7, np.uint64)
                env.lib.cc4o_rng_state(env._h, i, w.ctypes.data_as(ctypes.c_void_p))
                assert G.rng_words_match(f['rng'][t + 1], w), (f['name'], t)
        env.close()


# ---------------------------------------------------------------------------------------------------------------- 2. the rule
STEPS, CALLS, REASSIGN_AT, DEFAULT_AT = 30, 100, 10, 40


@pytest.mark.parametrize('rng_mode', [0, 1], ids=['numpy_stream', 'counter'])
def test_an_assignment_is_the_argument_of_the_next_regeneration(rng_mode, oracle_lib):
    """For each of the 16 class combinations A, with P and C two other combinations: episode `a` is regenerated with argument P and carries the
    assignment A; episode `b` carries none and is regenerated with the argument that should be in force.  Both take the same 100 random action rows
    through cc4o_step_batch(autoreset=1) on 30-step episodes -- done after 29 steps: regenerations in calls 30, 60 and 90.  At call 10 `a` is reassigned to C
    (mid-episode: nothing may change before the regeneration of call 30, which then gives C), at call 40 back to CC4_POLICY_DEFAULT (the
    regenerations of calls 60 and 90 give P).  Hot rows apart from the assignment byte and cold rows are equal after the reset and after every call."""
    at = M.assign_offset()
    for k, A in enumerate(M.COMBOS):
        P, C = M.COMBOS[(k + 5) % 16], M.COMBOS[(k + 11) % 16]
        assert len({A, P, C}) == 3
        a = OracleVecEnv(1, steps=STEPS, rng_mode=rng_mode, autoreset=True, red_policy=P[0], green_policy=P[1], blue_policy=P[2])
        b = OracleVecEnv(1, steps=STEPS, rng_mode=rng_mode, autoreset=True)
        assert a.policy == M.policy_bits(*P)
        M.oracle_assign(a, 0, *A)
        b.policy = M.policy_bits(*A)
        a.reset(seeds=700 + k), b.reset(seeds=700 + k)

        def same(where):
            ha, hb = a.get_state(0), b.get_state(0)
            assert hb[at] == 0, where
            ha[at] = 0
            assert np.array_equal(ha, hb), (A, where, np.nonzero(ha != hb)[0][:12].tolist())
            assert np.array_equal(a.get_cold(0), b.get_cold(0)), (A, where)

        same('reset')
        assert M.row_get(M.oracle_row(a, 0)) == (A, A) and M.row_get(M.oracle_row(b, 0)) == (A, (M.DEFAULT,) * 3)
        plan, _ = random_plan(np.random.default_rng(k), CALLS, 1)
        live_now, regens = A, 0
        for t in range(CALLS):
            if t == REASSIGN_AT:
                M.oracle_assign(a, 0, *C)
                b.policy = M.policy_bits(*C)
            if t == DEFAULT_AT:
                M.oracle_assign(a, 0, M.DEFAULT, M.DEFAULT, M.DEFAULT)
                b.policy = M.policy_bits(*P)
            was_done = bool(a._done[0])
            oa, ob = a.step_batch(plan[t]), b.step_batch(plan[t])
            for x, y in zip(oa[:3], ob[:3]):
                assert np.array_equal(x, y), (A, t)
            assert not oa[3]['err'].any() and not ob[3]['err'].any(), (A, t)
            same(t)
            if was_done:                     # this call regenerated the episode: the assignment (or the argument) as it stood took effect
                regens += 1
                live_now = C if REASSIGN_AT <= t < DEFAULT_AT else (P if t >= DEFAULT_AT else A)
            live, assigned = M.row_get(M.oracle_row(a, 0))
            assert live == live_now, (A, t, live, live_now)
            assert assigned == (A if t < REASSIGN_AT else C if t < DEFAULT_AT else (M.DEFAULT,) * 3), (A, t)
        assert regens == 3 and live_now == P
        a.close(), b.close()


# ---------------------------------------------------------------------------------------------------------------- 3. single rows
def test_row_policies_round_trip_and_refusals():
    nb = L_state_bytes()
    row = np.zeros(nb, np.uint8)
    assert M.row_get(row) == ((0, 0, 0), (M.DEFAULT,) * 3)              # a row that was never assigned
    at = M.assign_offset()
    for c in M.COMBOS:
        assert M.row_set(row, *c) == 0 and M.row_get(row) == ((0, 0, 0), c)
        assert np.count_nonzero(row) == 1 and row[at] == (0x80 | M.policy_bits(*c))      # one byte of the row, the encoding of EnvState.policy
    # a class at a time: the others stay; on a row without an assignment they come from the live classes
    assert M.row_set(row, 2, M.KEEP, M.KEEP) == 0 and M.row_get(row)[1] == (2, 1, 1)
    assert M.row_set(row, M.KEEP, 0, M.KEEP) == 0 and M.row_get(row)[1] == (2, 0, 1)
    assert M.row_set(row, M.KEEP, M.KEEP, M.KEEP) == 0 and M.row_get(row)[1] == (2, 0, 1)
    assert M.row_set(row, M.DEFAULT, M.KEEP, M.DEFAULT) == 0 and M.row_get(row)[1] == (M.DEFAULT,) * 3 and not row.any()
    ora = OracleVecEnv(1, steps=30, red_policy=3, green_policy=1)
    ora.reset(seeds=5)
    live = ora.get_state(0)
    assert M.row_get(live) == ((3, 1, 0), (M.DEFAULT,) * 3)
    assert M.row_set(live, M.KEEP, M.KEEP, 1) == 0 and M.row_get(live) == ((3, 1, 0), (3, 1, 1))
    ora.close()
    # refusals: -2, the row untouched
    assert M.row_set(row, 1, 1, 0) == 0
    before = row.copy()
    for bad in ((4, 0, 0), (0, 2, 0), (0, 0, 2), (-3, 0, 0), (0, -3, 0), (0, 0, 127), (M.DEFAULT, 1, M.KEEP), (1, M.KEEP, M.DEFAULT), (256, 0, 0)):
        assert M.row_set(row, *bad) == -2, bad
        assert np.array_equal(row, before), bad
    lib = M.L.load()
    assert lib.cc4_row_set_policies(None, 0, 0, 0) == -2 and lib.cc4_row_get_policies(None, None, None) == -2


def L_state_bytes():
    return int(M.L.load().cc4_state_bytes())


def test_python_surface_is_declared():
    from cage_challenge_4_amd import CC4VecEnv, _lib
    for name in ('cc4_set_policies_device', 'cc4_set_policies', 'cc4_policies_device', 'cc4_get_policies', 'cc4_row_set_policies',
                 'cc4_row_get_policies', 'cc4_reset_device'):
        assert name in _lib.SIGNATURES and hasattr(_lib.load(), name), name
    assert callable(getattr(CC4VecEnv, 'set_policies', None)) and callable(getattr(CC4VecEnv, 'policies', None))
    assert (_lib.POLICY_KEEP, _lib.POLICY_DEFAULT) == (-1, -2)
