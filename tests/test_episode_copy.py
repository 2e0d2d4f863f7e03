"""GPU: episode copies on the device (cc4_copy_episodes_device through CC4VecEnv.clone_episodes): a clone behaves as its source -- against the
reference's golden trajectories in both RNG modes, and against the CPU oracle's host snapshot / restore at the bench batch -- its reseed is
cc4_set_seed's, and faulty entries are skipped and reported while the others apply."""
import numpy as np
import pytest
import golden_util as G
from oracle_binding import OracleVecEnv, random_actions

pytestmark = pytest.mark.gpu


@pytest.fixture(params=[0, 1], ids=['4wave', '1wave'])
def philox_kernel(request, monkeypatch):
    """Both counter-mode step kernels (test_hip_parity.philox_kernel's parametrisation)."""
    monkeypatch.setenv('CC4_PHILOX_LEAN', str(request.param))
    return ('k_step_philox', 'k_step_philox1')[request.param]


def _poison_dead_bytes(env, e):
    """Every cold byte of episode e becomes 0xA5 (cc4_set_cold alone: no full observation rewrite is forced): a copy onto e rewrites the live
    extents, and whatever reads a dead byte afterwards sees garbage."""
    import ctypes
    cold = np.full(env.lib.cc4_cold_bytes(env._h), 0xA5, np.uint8)
    env._chk(env.lib.cc4_set_cold(env._h, int(e), cold.ctypes.data_as(ctypes.c_void_p)), 'cc4_set_cold')


def _schedule(T):
    return T // 3, (2 * T) // 3


def _check(env, fix, e, t, obs, rew, done, st=None, what=''):
    assert np.array_equal(obs[e], fix['obs'][t]), (fix['name'], what, e, t)
    if rew is not None:
        assert rew[e] == fix['reward'][t - 1] and bool(done[e]) == bool(fix['done'][t - 1]), (fix['name'], what, e, t)
    if st is not None and 'rng' in fix:
        assert G.rng_words_match(fix['rng'][t], st[e]), (fix['name'], what, e, t)


def _replay_with_clones(env, fixes, partner_actions, k, rng_words):
    """Episodes 0..k-1 follow the fixtures, k..2k-1 are their partners (a heavier action script).  At T/3 each golden episode is cloned onto
    its partner (whose dead bytes are poisoned first); the clone follows the fixture from then on and the golden slot runs the partner's
    script.  At 2T/3 the clone goes back onto the golden slot (poisoned as well); both follow the fixture to the end.  Every step of
    whichever episode follows the fixture is compared: observations, reward, done, (numpy stream) the PCG64 position; masks after each clone."""
    T = fixes[0]['actions'].shape[0]
    c1, c2 = _schedule(T)
    gold = np.arange(k)                  # slot that follows the fixture: before c1 and after c2 the original one, in between the clone
    zero_m = np.zeros((5, 8), np.uint8)
    for t in range(T):
        if t in (c1, c2):
            src = gold if t == c1 else gold + k
            dst = gold + k if t == c1 else gold
            for e in dst:
                _poison_dead_bytes(env, int(e))
            obs = env.clone_episodes(src, dst).copy()
            st = env.rng_state() if rng_words else None
            mask = env.action_mask
            for i, f in enumerate(fixes):
                _check(env, f, int(dst[i]), t, obs, None, None, st, 'after clone')
                assert np.array_equal(mask[dst[i]], f['mask']), (f['name'], t)
        follow = set(range(k)) if t < c1 or t >= c2 else set(range(k, 2 * k))
        if t >= c2:
            follow |= set(range(k, 2 * k))
        a = np.zeros((2 * k, 5), np.int32)
        m = np.zeros((2 * k, 5, 8), np.uint8)
        for e in range(2 * k):
            f = fixes[e % k]
            if e in follow:
                a[e] = f['actions'][t]
                m[e] = f['messages'][t] if f['messages'] is not None else zero_m
            else:
                a[e] = partner_actions[t % partner_actions.shape[0]]
        obs, rew, done, info = env.step(a, m)
        st = env.rng_state() if rng_words else None
        for e in sorted(follow):
            _check(env, fixes[e % k], e, t + 1, obs, rew, done, st)
        assert not info['err'].any(), t


def _heavy(fixes_all, steps):
    """the decoy-stacking fixture of that length: its episodes' process lists overflow into the cold row (povf)"""
    return [f for f in fixes_all if f['steps'] == steps and 'decoy_one' in f['name']][0]['actions']


def test_reference_trajectories_survive_clones_numpy_stream():
    from cage_challenge_4_amd import CC4VecEnv
    allf = [G.load(p) for p in G.list_fixtures()]
    todo = [f for f in allf if f['steps'] in (500, 1000)]
    names = {f['name'] for f in todo}
    assert 'traj_seed321_decoy_one_ctor_500.npz' in names and 'traj_seed777_decoy_one_ctor_1000.npz' in names
    groups = {}
    for f in todo:
        groups.setdefault((f['steps'], f['red_policy'], f['green_policy'], f['blue_policy']), []).append(f)
    for (steps, rp, gp, bp), fixes in sorted(groups.items(), key=lambda kv: kv[0]):
        k = len(fixes)
        env = CC4VecEnv(2 * k, steps=steps, red_policy=rp, green_policy=gp, blue_policy=bp)
        seeds = np.array([f['seed'] for f in fixes] + [f['seed'] + 7919 for f in fixes], np.uint64)
        env.reset(seeds=seeds)
        ctor = np.array([f['reset_seed'] < 0 for f in fixes] * 2, np.uint8)
        env.reset(seeds=None, env_mask=ctor)
        second = np.array([max(f['reset_seed'], 0) for f in fixes] + [f['seed'] + 104729 for f in fixes], np.uint64)
        obs = env.reset(seeds=second, env_mask=1 - ctor)
        for i, f in enumerate(fixes):
            assert np.array_equal(obs[i], f['obs'][0]) and np.array_equal(env.action_mask[i], f['mask']), f['name']
        _replay_with_clones(env, fixes, _heavy(allf, steps), k, rng_words=True)
        env.close()


def test_counter_mode_trajectories_survive_clones(philox_kernel):
    from cage_challenge_4_amd import CC4VecEnv
    allf = [G.load_ctr(p) for p in G.list_ctr_fixtures()]
    for steps in (500, 1000):
        fixes = [f for f in allf if f['steps'] == steps]
        k = len(fixes)
        env, obs0, masks = G.ctr_start(CC4VecEnv, fixes + fixes)      # partners start as the fixture's scenario, then take the heavy script
        assert env.step_kernel == philox_kernel
        for i, f in enumerate(fixes):
            assert np.array_equal(obs0[i], f['obs'][0]) and np.array_equal(masks[i], f['mask']), f['name']
        _replay_with_clones(env, fixes, _heavy(allf, steps), k, rng_words=False)
        env.close()


@pytest.mark.parametrize('run_kernel', ['k_run_philox1', 'per_step'])
def test_clones_at_the_bench_batch_match_host_restore_on_the_oracle(run_kernel):
    """8192 counter-mode episodes with autoreset, as bench.py runs them.  At several points random disjoint sets of episodes are cloned on the
    device, and restore(dst, snapshot(src)) does the same on the oracle; run_random_steps (the persistent kernel, or per-step launches in calls of
    fewer than ten steps) against the oracle's step_batch, outputs after every region, hot rows of every episode and true-state documents of a
    sample of destinations at the end."""
    from cage_challenge_4_amd import CC4VecEnv
    n, steps, seed0 = 8192, 500, 77
    dev = CC4VecEnv(n, steps=steps, rng_mode=1, autoreset=True, strict=False)
    ora = OracleVecEnv(n, steps=steps, rng_mode=1, autoreset=True, strict=False)
    assert np.array_equal(dev.reset(seeds=seed0), ora.reset_batch(seed0))
    region, regions = (30, 6) if run_kernel == 'k_run_philox1' else (6, 20)
    assert dev.run_kernel_for(region) == (run_kernel if run_kernel != 'per_step' else dev.step_kernel)
    rng = np.random.default_rng(5)
    t, all_dst = 0, set()
    for r in range(regions):
        if r > 0:
            perm = rng.permutation(n)
            m = int(rng.integers(16, 256))
            src, dst = perm[:m].astype(np.int32), perm[m:2 * m].astype(np.int32)
            for s, d in zip(src, dst):
                ora.restore(int(d), ora.snapshot(int(s)))
                ora._obs[d], ora._rew[d], ora._done[d], ora._err[d] = ora._obs[s], ora._rew[s], ora._done[s], ora._err[s]
            obs = dev.clone_episodes(src, dst)
            assert np.array_equal(obs, ora._obs), r
            assert np.array_equal(dev.action_mask[dst], dev.action_mask[src]), r
            all_dst |= set(dst.tolist())
        dev.run_random_steps(seed0, t, region, timed=False)
        for j in range(region):
            ora.step_batch(random_actions(seed0, t + j, n))
        t += region
        dev._fetch()
        bad = np.nonzero((dev._obs != ora._obs).any(axis=1) | (dev._rew != ora._rew) | (dev._done.astype(bool) != ora._done) | (dev._err != ora._err))[0]
        assert bad.size == 0, (r, bad[:10].tolist())
    assert t >= 120
    hot = dev.get_states()
    for i in range(n):
        assert np.array_equal(hot[i], ora.get_state(i)), i
    for e in sorted(all_dst)[::97]:
        assert dev.true_state_json(e) == ora.true_state_json(e), e
    dev.close()
    ora.close()


@pytest.mark.parametrize('rng_mode', [0, 1], ids=['pcg64', 'philox'])
def test_reseeded_clone_is_restore_then_set_seed(rng_mode):
    """deepcopy(env); env.set_seed(s): the oracle restores the source into a one-episode scratch handle, set_seed([s]) there, and the result
    goes onto the destination.  40 steps after: outputs, generator words, hot rows."""
    from cage_challenge_4_amd import CC4VecEnv
    n, steps = 12, 500
    dev = CC4VecEnv(n, steps=steps, rng_mode=rng_mode)
    ora = OracleVecEnv(n, steps=steps, rng_mode=rng_mode)
    scratch = OracleVecEnv(1, steps=steps, rng_mode=rng_mode)
    dev.reset(seeds=900)
    ora.reset(seeds=900)
    for t in range(25):
        dev.step(random_actions(900, t, n))
        ora.step(random_actions(900, t, n))
    src, dst = np.array([0, 1, 2, 2], np.int32), np.array([5, 6, 7, 8], np.int32)
    seeds = np.array([11, 12, 13, 14], np.uint64)
    dev.clone_episodes(src, dst, seeds)
    for s, d, sd in zip(src, dst, seeds):
        scratch.restore(0, ora.snapshot(int(s)))
        scratch.set_seed(np.array([sd], np.uint64))
        ora.restore(int(d), scratch.snapshot(0))
    assert np.array_equal(dev.rng_state(), ora.rng_state())
    for t in range(25, 65):
        d = dev.step(random_actions(901, t, n))
        o = ora.step(random_actions(901, t, n))
        assert np.array_equal(d[0], o[0]) and np.array_equal(d[1], o[1]) and np.array_equal(d[2], o[2]), t
    assert np.array_equal(dev.rng_state(), ora.rng_state())
    for i in range(n):
        assert np.array_equal(dev.get_state(i), ora.get_state(i)), i
    dev.close()
    ora.close()
    scratch.close()


def test_faulty_entries_are_skipped_and_reported():
    """An index out of range, a duplicated destination, a destination that is also a source: each raises CC4EngineError naming it; the
    faulty entries' destinations keep their rows, the valid entries of the same call apply."""
    from cage_challenge_4_amd import CC4VecEnv
    from cage_challenge_4_amd.vec_env import CC4EngineError
    n = 16
    env = CC4VecEnv(n, steps=100, rng_mode=1)
    env.reset(seeds=np.arange(100, 100 + n, dtype=np.uint64))
    for t in range(7):
        env.step(random_actions(3, t, n))
    cases = [('INDEX_OUT_OF_RANGE', [0, 1, -1], [2, n, 3]),              # (1 -> n) and (-1 -> 3) out of range; 0 -> 2 valid
             ('DUPLICATED_DESTINATION', [0, 1, 4], [5, 5, 6]),           # both entries naming 5 skipped; 4 -> 6 valid
             ('SOURCE_IS_DESTINATION', [0, 7, 9], [7, 8, 9])]            # 7 is a destination (0 -> 7 valid, 7 -> 8 skipped), 9 -> 9 skipped
    for name, src, dst in cases:
        before = env.get_states()
        with pytest.raises(CC4EngineError, match=name):
            env.clone_episodes(np.array(src), np.array(dst))
        after = env.get_states()
        applied = {d: s for s, d in zip(src, dst) if 0 <= s < n and 0 <= d < n and dst.count(d) == 1 and s not in dst}
        for e in range(n):
            want = before[applied[e]] if e in applied else before[e]
            assert np.array_equal(after[e], want), (name, e)
        assert applied, name
    env.clone_episodes(np.array([1]), np.array([2]))                   # a clean call raises nothing: the faults were cleared
    env.close()


def test_no_copy_on_a_handle_with_a_communicator_or_during_a_rollout():
    import ctypes
    import os
    from cage_challenge_4_amd import CC4VecEnv
    from cage_challenge_4_amd._lib import CC4Error
    env = CC4VecEnv(8192, steps=50, rng_mode=1)
    env.reset(seeds=4)
    lib, h = env.lib, env._h
    K = 4
    assert env.run_kernel_for(20) == 'k_run_philox1'
    assert lib.cc4_rollout_begin(h, K) == 0, lib.cc4_last_error(h)
    idx = np.array([0, 1], np.int32)
    assert lib.cc4_clone_episodes(h, 1, idx.ctypes.data_as(ctypes.c_void_p), idx[1:].ctypes.data_as(ctypes.c_void_p), None) == -2
    assert b'rollout' in lib.cc4_last_error(h)
    G_, blk = ctypes.c_int32(), ctypes.c_int32()
    rc = lib.cc4_rollout_groups(h, ctypes.byref(G_), ctypes.byref(blk))
    s0 = ctypes.c_uint64(4)
    for j in range(K):
        for g in range(G_.value):
            rc = rc or lib.cc4_rollout_sync(h, g if j > 0 else -1, j - 1, g, j, None)
            rc = rc or lib.cc4_rollout_random_policy(h, g, j, s0, ctypes.c_uint32(j), None)
    for g in range(G_.value):
        rc = rc or lib.cc4_rollout_sync(h, g, K - 1, -1, 0, None)
    assert lib.cc4_rollout_end(h) == 0 and rc == 0, lib.cc4_last_error(h)
    env.clone_episodes(np.array([0]), np.array([1]))                   # after the rollout: fine
    env.close()
    one = CC4VecEnv(4, steps=50, rng_mode=1)
    one.reset(seeds=5)
    os.environ.setdefault('NCCL_SOCKET_IFNAME', 'lo')
    ident = (ctypes.c_uint8 * 128)()
    assert one.lib.cc4_comm_unique_id(ident) == 0
    one._chk(one.lib.cc4_comm_init(one._h, 0, 1, ident), 'cc4_comm_init')
    with pytest.raises(CC4Error, match='communicator'):
        one.clone_episodes(np.array([0]), np.array([1]))
    one.close()
