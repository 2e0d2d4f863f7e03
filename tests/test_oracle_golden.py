"""CPU: the oracle (host build of the engine restatement) against the golden trajectories recorded from the REAL
reference (oracle/refgen/make_golden.py).  Bit-exact: flat observations, team reward, done, action mask and the
numpy PCG64 stream position after every step."""
import numpy as np
import pytest
import golden_util as G
from oracle_binding import OracleVecEnv


def replay(env_cls, fix, **kw):
    env = env_cls(1, steps=fix['steps'], **kw)
    if fix['reset_seed'] < 0:          # CybORG(seed=s); wrapper.reset()
        env.reset(seeds=np.array([fix['seed']], np.uint64))
        obs = env.reset(seeds=None)
    else:                              # wrapper.reset(seed=s+1)
        env.reset(seeds=np.array([fix['seed']], np.uint64))
        obs = env.reset(seeds=np.array([fix['reset_seed']], np.uint64))
    return env, obs


@pytest.mark.parametrize('path', G.list_fixtures(), ids=lambda p: p.split('/')[-1])
def test_oracle_matches_reference_trajectory(path, oracle_lib):
    fix = G.load(path)
    env, obs = replay(OracleVecEnv, fix, red_policy=fix['red_policy'], green_policy=fix['green_policy'], blue_policy=fix['blue_policy'])
    assert np.array_equal(obs[0], fix['obs'][0])
    assert np.array_equal(env.mask()[0], fix['mask'])
    assert G.rng_words_match(fix['rng'][0], env.rng_state()[0])
    T = fix['actions'].shape[0]
    total = 0.0
    for t in range(T):
        m = None if fix['messages'] is None else fix['messages'][t][None]
        obs, rew, done, info = env.step(fix['actions'][t][None], m)
        assert np.array_equal(obs[0], fix['obs'][t + 1]), f'obs differs at step {t}'
        assert rew[0] == fix['reward'][t], f'reward differs at step {t}'
        assert bool(done[0]) == bool(fix['done'][t]), f'done differs at step {t}'
        assert G.rng_words_match(fix['rng'][t + 1], env.rng_state()[0]), f'PCG64 stream position differs at step {t}'
        assert info['err'][0] == 0
        total += float(rew[0])
    assert total == float(fix['reward'].sum())
    env.close()


# ---------------------------------------------------------------------------------------------------------------- the stand-in fixtures
# ctrstand_*.npz / trajstand_*.npz: reference episodes whose blue actions are the draws cc4_run_random_steps makes in the kernel (golden_util.STANDIN_BASE)
def test_standin_fixture_set():
    """Nine counter-mode fixtures at the offsets the placement tests rely on, three numpy-stream ones; every red class, both green classes, a dynamics
    key with a high word, action keys with a high word, scenario seeds no other fixture uses, 100-step episodes."""
    import standin_util as S
    ctr, pcg = S.fixtures(1), S.fixtures(0)
    assert tuple(f['d'] for f in ctr) == G.STANDIN_OFFSETS and tuple(f['d'] for f in pcg) == (0, 64, 1023)
    assert G.STANDIN_BASE >> 32 and all(f['akey'] >> 32 for f in ctr + pcg)
    assert {f['red_policy'] for f in ctr} == {0, 1, 2, 3} and {f['green_policy'] for f in ctr} == {0, 1}
    assert any(f['key'] >> 32 for f in ctr)
    assert [f['red_policy'] for f in pcg] == [0, 2, 3]
    others = {f['seed'] for f in map(G.load, G.list_fixtures())} | {f['seed'] for f in map(G.load_ctr, G.list_ctr_fixtures())}
    seeds = [f['seed'] for f in ctr + pcg]
    assert len(set(seeds)) == len(seeds) and not set(seeds) & others
    assert all(f['steps'] == 100 and f['obs'].shape == (101, 578) for f in ctr + pcg)
    for f in ctr + pcg:          # all three mission phases (33 / 33 / 34 steps), in order, and the episode ends with the last step
        phase = f['obs'][:, 0]
        assert set(phase.tolist()) == {0, 1, 2} and (np.diff(phase) >= 0).all() and (np.bincount(phase) >= 33).all(), f['name']
        assert f['done'][-1] and not f['done'][:90].any(), f['name']


@pytest.mark.parametrize('mode', [1, 0], ids=['counter', 'numpy-stream'])
def test_standin_fixture_actions_are_the_stand_in_draws(mode):
    """The stored actions are random_blue_action(akey, t, 0, agent), and the fixture with akey = STANDIN_BASE + d holds the draws of slot d of a batch stepped
    with seed0 = STANDIN_BASE (the placement rule: slot e of a batch draws from key seed0 + e)."""
    import standin_util as S
    from oracle_binding import random_actions
    fx = S.fixtures(mode)
    deepest = max(f['d'] for f in fx)
    for t in range(S.STEPS):
        batch = random_actions(G.STANDIN_BASE, t, deepest + 1)
        for f in fx:
            assert np.array_equal(f['actions'][t], random_actions(f['akey'], t, 1)[0]), (f['name'], t)
            assert np.array_equal(f['actions'][t], batch[f['d']]), (f['name'], t)
    assert all((f['actions'] >= 0).all() and (f['actions'][:, :4] < 82).all() and (f['actions'][:, 4] < 242).all() for f in fx)


@pytest.mark.parametrize('mode', [1, 0], ids=['counter', 'numpy-stream'])
def test_oracle_matches_reference_on_the_standin_fixtures(mode, oracle_lib):
    """Every stand-in fixture replays on the oracle at every step: observations, reward, done, no error flag, (first observations and masks:
    standin_util._oracle_start) and the PCG64 stream position for the numpy-stream files."""
    import standin_util as S
    ora = S.oracle_replay(mode)
    for f in S.fixtures(mode):
        r = ora[f['name']]
        for t in range(S.STEPS + 1):
            assert np.array_equal(r['obs'][t], f['obs'][t]), (f['name'], 'observations after step', t - 1)
            if mode == 0:
                assert G.rng_words_match(f['rng'][t], r['rng'][t]), (f['name'], 'PCG64 stream position after step', t - 1)
        assert np.array_equal(r['reward'], f['reward']), (f['name'], np.nonzero(r['reward'] != f['reward'])[0][:4])
        assert np.array_equal(r['done'], f['done']) and not r['err'].any(), f['name']
        assert sorted(r['hot']) == list(S.ENDS)


def test_baseline_config1_episode_rewards(oracle_lib):
    # seed 123 -> -5634, seed 7 -> -4154 (SleepAgent blue, 500 steps)
    want = {'traj_seed123_sleep_ctor_500.npz': -5634.0, 'traj_seed7_sleep_ctor_500.npz': -4154.0}
    for p in G.list_fixtures():
        name = p.split('/')[-1]
        if name in want:
            assert float(G.load(p)['reward'].sum()) == want[name]


def test_oracle_counter_mode_matches_reference_under_the_philox_proxy(oracle_lib):
    """the counter (Philox) mode's STEP pinned to reference trajectories.  tests/golden/ctrstep_*.npz were
    recorded from the real reference stepping under oracle/refgen/philox_proxy.PhiloxProxy -- a Generator stand-in passed as
    CybORG(seed=proxy) that serves every draw of the step path from the engine's (draw, stream, step, episode) Philox words,
    the stream identified from the call site -- on scenarios generated from the numpy stream on both sides.  Every step's
    observations, reward and done flag of ten episodes (random / structured / built-in blue, three red policies, both green
    policies, messages) must match."""
    import ctypes
    from oracle_binding import OracleVecEnv
    allf = [G.load_ctr(p) for p in G.list_ctr_fixtures()]
    assert len(allf) >= 10 and sum(f['steps'] == 500 for f in allf) >= 9 and {f['red_policy'] for f in allf} == {0, 2, 3}
    for steps in sorted({f['steps'] for f in allf}):
        fixes = [f for f in allf if f['steps'] == steps]
        env, obs0, masks = G.ctr_start(OracleVecEnv, fixes)
        for i, f in enumerate(fixes):
            assert np.array_equal(obs0[i], f['obs'][0]) and np.array_equal(masks[i], f['mask']), f['name']
        for t in range(steps):
            for i, f in enumerate(fixes):
                a = np.ascontiguousarray(f['actions'][t], np.int32)
                m = np.ascontiguousarray(f['messages'][t] if f['messages'] is not None else np.zeros((5, 8), np.uint8))
                env.lib.cc4o_step(env._h, i, a.ctypes.data_as(ctypes.c_void_p), m.ctypes.data_as(ctypes.c_void_p))
                env._collect(i)
                assert np.array_equal(env._obs[i], f['obs'][t + 1]), (f['name'], t)
                assert env._rew[i] == f['reward'][t] and bool(env._done[i]) == bool(f['done'][t]), (f['name'], t)
                assert env._err[i] == 0, (f['name'], t)
        env.close()
