"""GPU: per-episode opponent classes (cc4_set_policies / CC4VecEnv.set_policies) and their regenerations.  Every comparison is exact.
4. ONE numpy-stream handle of default configuration replays the reference trajectories of every class combination from assignments alone;
5. a handle with red class e % 4 assigned to episode e == four uniform handles, in every step, run and plan kernel, and under the self-check;
6. all 16 class combinations and a reassignment in mid-episode against the oracle, whose rows are edited the same way;
8. clones carry live classes and assignments; out-of-range values are skipped and reported; refusals inside a rollout."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

import golden_util as G
import mix_util as M
from oracle_binding import OracleVecEnv, random_actions
from plan_util import random_plan

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STEPS, CALLS = 30, 100          # 30-step episodes with autoreset: done after 29 steps, so the calls 30, 60 and 90 regenerate every episode


def _env(n, **kw):
    from cage_challenge_4_amd import CC4VecEnv
    kw.setdefault('strict', False)
    return CC4VecEnv(n, **kw)


def _twin(monkeypatch, n, **kw):
    """A further device handle as tests/test_plan.py builds its twins: ONE stream (CC4_GROUPS=1) and no sampled self-check shadow."""
    monkeypatch.setenv('CC4_GROUPS', '1')
    monkeypatch.setenv('CC4_PERSIST_VERIFY_EVERY', '0')
    try:
        return _env(n, **kw)
    finally:
        monkeypatch.delenv('CC4_GROUPS')
        monkeypatch.delenv('CC4_PERSIST_VERIFY_EVERY')


# ---------------------------------------------------------------------------------------------------------------- 4. reference-anchored
def test_one_default_handle_replays_the_reference_trajectories_of_every_class():
    """All 500-step traj_* fixtures -- reddiscovery and the built-in blue among them -- in ONE numpy-stream handle created with the default classes,
    each episode assigned its fixture's; seeded as test_hip_matches_reference_golden_trajectories seeds them (the ctor fixtures' second reset(None) is
    itself a regeneration under the assignment).  Every step against the recorded arrays, the PCG64 position included."""
    fixes = [f for f in map(G.load, G.list_fixtures()) if f['steps'] == 500]
    classes = np.array([(f['red_policy'], f['green_policy'], f['blue_policy']) for f in fixes], np.int8)
    assert len(fixes) >= 12 and (classes != 0).any(axis=1).sum() >= 2, classes.tolist()
    n = len(fixes)
    env = _env(n, steps=500, strict=True)
    env.set_policies(red=classes[:, 0], green=classes[:, 1], blue=classes[:, 2])
    env.reset(seeds=np.array([f['seed'] for f in fixes], np.uint64))
    ctor = np.array([f['reset_seed'] < 0 for f in fixes], np.uint8)
    env.reset(seeds=None, env_mask=ctor)                               # CybORG(seed); wrapper.reset()
    second = np.array([max(f['reset_seed'], 0) for f in fixes], np.uint64)
    obs = env.reset(seeds=second, env_mask=1 - ctor)                  # wrapper.reset(seed=s+1)
    live, assigned = env.policies()
    assert np.array_equal(live, classes) and np.array_equal(assigned, classes)
    for i, f in enumerate(fixes):
        assert np.array_equal(obs[i], f['obs'][0]), f['name']
        assert np.array_equal(env.action_mask[i], f['mask']), f['name']
    for t in range(500):
        a = np.stack([f['actions'][t] for f in fixes])
        m = np.stack([f['messages'][t] if f['messages'] is not None else np.zeros((5, 8), np.uint8) for f in fixes])
        obs, rew, done, info = env.step(a, m)
        st = env.rng_state()
        for i, f in enumerate(fixes):
            assert np.array_equal(obs[i], f['obs'][t + 1]), (f['name'], t)
            assert rew[i] == f['reward'][t], (f['name'], t)
            assert bool(done[i]) == bool(f['done'][t]), (f['name'], t)
            assert G.rng_words_match(f['rng'][t + 1], st[i]), (f['name'], t)
        assert not info['err'].any()
    env.close()


# ---------------------------------------------------------------------------------------------------------------- 5. mixed == uniform
# (id, batch, rng_mode, CC4_PHILOX_LEAN, how the 100 steps are taken, the kernel the handle names for it).  The smallest batches that name each
# form: 64 episodes -- 16 per class -- for what a small handle runs, 6656 for the persistent forms (as the existing tests reach them).
FORMS = [
    ('k_step', 64, 0, None, 'plan', 'k_step'),
    ('k_step_philox', 1024, 1, '0', 'plan', 'k_step_philox'),
    ('k_step_philox1', 1024, 1, '1', 'plan', 'k_step_philox1'),
    ('k_run_philox', 64, 1, '0', 'run', 'k_run_philox'),
    ('k_run_philox1m', 64, 1, '1', 'run', 'k_run_philox1m'),
    ('k_run_philox1', 6656, 1, None, 'run', 'k_run_philox1'),
    ('k_run_philox1p', 6656, 1, None, 'plan', 'k_run_philox1p'),
    ('k_run_pcg', 6656, 0, None, 'run', 'k_run_pcg'),
    ('k_run_pcgp', 6656, 0, None, 'plan', 'k_run_pcgp'),
]
BURST = 10                      # 'run': cc4_run_random_steps in calls of 10 steps (the persistent forms' shortest), outputs compared after each


def _drive(env, how, kernel, plan, seed0):
    """The 100 steps on one handle.  Returns what they left behind per step (plan calls: rewards, dones, packed observations of every step; run calls:
    observations, rewards, dones after every burst) and at the end (outputs, masks, error words, generator words, hot rows of a sample)."""
    n = env.num_envs
    if how == 'plan':
        assert env.plan_kernel_for(CALLS) == kernel, env.plan_kernel_for(CALLS)
        per_step = M.run_plan_packed(env, plan)
    else:
        assert env.run_kernel_for(BURST) == kernel, env.run_kernel_for(BURST)
        seq = []
        for t in range(0, CALLS, BURST):
            env.run_random_steps(seed0, t, BURST, timed=False)
            seq.append(M.final_outputs(env)[:3])
        per_step = tuple(np.stack(x) for x in zip(*seq))
    sample = sorted(set(range(0, min(n, 16))) | set(range(n - 8, n)) | {n // 2 + c for c in range(4)})
    rows = np.stack([env.get_state(i) for i in sample])
    return per_step, M.final_outputs(env), env.rng_state(), sample, rows


@pytest.mark.parametrize('form', FORMS, ids=lambda f: f[0])
def test_mixed_handle_equals_uniform_handles(form, monkeypatch):
    """Episode e of the mixed handle is assigned red class e % 4 before its first reset; four uniform handles are created with red_policy = c, one after
    the other, and given the same seeds and the same 100 steps.  The episodes with e % 4 == c must be uniform handle c's, step by step and at the end
    (hot rows apart from the assignment byte), across three regenerations inside the calls."""
    name, n, mode, lean, how, kernel = form
    if lean is not None:
        monkeypatch.setenv('CC4_PHILOX_LEAN', lean)
    seed0 = 5100 + n + mode
    plan, _ = random_plan(np.random.default_rng(seed0), CALLS, n)
    cls = (np.arange(n) % 4).astype(np.int8)
    mixed = _env(n, steps=STEPS, rng_mode=mode, autoreset=True, red_policy=cls)
    live, assigned = mixed.policies()
    assert not live.any() and np.array_equal(assigned[:, 0], cls) and not assigned[:, 1:].any()      # assigned before the first reset, nothing live yet
    mixed.reset(seeds=seed0)
    assert np.array_equal(mixed.policies()[0][:, 0], cls)
    got = _drive(mixed, how, kernel, plan, seed0)
    live, assigned = mixed.policies()
    assert np.array_equal(live[:, 0], cls) and np.array_equal(assigned[:, 0], cls)
    mixed.close()
    assert not got[1][3].any()                                       # no error word
    for c in range(4):
        uni = _twin(monkeypatch, n, steps=STEPS, rng_mode=mode, autoreset=True, red_policy=c)
        uni.reset(seeds=seed0)
        want = _drive(uni, how, kernel, plan, seed0)
        live, assigned = uni.policies()
        assert (live[:, 0] == c).all() and (assigned == M.DEFAULT).all()
        uni.close()
        mine = cls == c
        for j, what in enumerate(('rewards', 'dones', 'packed observations') if how == 'plan' else ('observations', 'rewards', 'dones')):
            x, y = got[0][j][:, mine], want[0][j][:, mine]
            assert np.array_equal(x, y), (name, c, what, np.argwhere(x != y)[:4].tolist())
        if how == 'plan':
            d = want[0][1]
            assert (d.sum(axis=0) >= 3).all()                        # every episode ended -- and was regenerated in the next call -- three times
        for j, what in enumerate(('final observations', 'final reward', 'final done', 'error words', 'masks')):
            assert np.array_equal(got[1][j][mine], want[1][j][mine]), (name, c, what)
        assert np.array_equal(got[2][mine], want[2][mine]), (name, c, 'generator words')
        assert got[3] == want[3]
        pick = [k for k, e in enumerate(got[3]) if e % 4 == c]
        assert len(pick) >= 4
        a, b = M.without_assignment(got[4][pick]), want[4][pick]
        assert np.array_equal(a, b), (name, c, 'hot rows', np.argwhere(a != b)[:6].tolist())
        at = M.assign_offset()
        assert (got[4][pick][:, at] == (0x80 | c)).all() and not want[4][pick][:, at].any()


_VERIFY_CHILD = r'''
import sys
import numpy as np
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, sys.argv[1] + '/tests')
from cage_challenge_4_amd import CC4VecEnv
from plan_util import random_plan
n = 6656
cls = (np.arange(n) % 4).astype(np.int8)
for mode in (1, 0):
    env = CC4VecEnv(n, steps=30, rng_mode=mode, autoreset=True, strict=False, red_policy=cls)
    env.reset(seeds=77)
    assert env.run_kernel_for(40).startswith('k_run_') and env.plan_kernel_for(40).startswith('k_run_')
    env.run_random_steps(77, 0, 40, timed=False)
    env.run_plan(random_plan(np.random.default_rng(mode), 40, n)[0])
    env.run_random_steps(77, 80, 25, timed=False)
    checked, bad = env.verify_stats()
    live, assigned = env.policies()
    assert np.array_equal(live[:, 0], cls) and np.array_equal(assigned[:, 0], cls)
    assert not env.err.any()
    print('VERIFY', mode, checked, bad)
    env.close()
'''


def test_self_check_shadow_regenerates_as_the_mixed_handle_does():
    """CC4_PERSIST_VERIFY=1 in a child process: every one-launch call of a mixed handle (run and plan, both RNG modes, 105 steps of 30-step episodes) is
    repeated with per-step launches on the shadow handle -- created with the handle's default classes, seeded with its rows -- and compared."""
    env = dict(os.environ, CC4_PERSIST_VERIFY='1')
    pr = subprocess.run([sys.executable, '-c', _VERIFY_CHILD, ROOT], env=env, capture_output=True, text=True, timeout=300)
    assert pr.returncode == 0, pr.stdout[-2000:] + pr.stderr[-4000:]
    lines = [ln.split() for ln in pr.stdout.splitlines() if ln.startswith('VERIFY')]
    assert len(lines) == 2, pr.stdout
    for _, mode, checked, bad in lines:
        assert int(checked) == 3 and int(bad) == 0, (mode, checked, bad)


# ---------------------------------------------------------------------------------------------------------------- 6. green, blue, timing
@pytest.mark.parametrize('mode,lean', [(0, None), (1, '0'), (1, '1')], ids=['numpy_stream', 'counter_four_wave', 'counter_one_wave'])
def test_all_class_combinations_and_a_reassignment_against_the_oracle(mode, lean, monkeypatch):
    """64 episodes on a handle of default configuration, episode e assigned combination e % 16 before the first reset and combination (e + 5) % 16 at
    step 10 of its 30-step episode; the oracle's rows are edited the same way and its regenerations get the default argument.  Every step of 100
    equals the oracle's; the live classes stay until the regeneration of call 30 and are the new ones afterwards."""
    if lean is not None:
        monkeypatch.setenv('CC4_PHILOX_LEAN', lean)
    n = 64
    first = np.array([M.COMBOS[e % 16] for e in range(n)], np.int8)
    then = np.array([M.COMBOS[(e + 5) % 16] for e in range(n)], np.int8)
    dev = _env(n, steps=STEPS, rng_mode=mode, autoreset=True)
    ora = OracleVecEnv(n, steps=STEPS, rng_mode=mode, autoreset=True)
    dev.set_policies(*first.T)
    for e in range(n):
        M.oracle_assign(ora, e, *first[e])
    assert np.array_equal(dev.reset(seeds=880 + mode), ora.reset(seeds=880 + mode))
    assert np.array_equal(dev.action_mask, ora.mask())
    plan, _ = random_plan(np.random.default_rng(mode), CALLS, n)
    for t in range(CALLS):
        if t == 10:
            dev.set_policies(red=then[:, 0], green=then[:, 1], blue=then[:, 2])
            for e in range(n):
                M.oracle_assign(ora, e, *then[e])
        d, o = dev.step(plan[t]), ora.step_batch(plan[t])
        assert np.array_equal(d[0], o[0]) and np.array_equal(d[1], o[1]) and np.array_equal(d[2], o[2]), t
        assert not d[3]['err'].any() and not o[3]['err'].any(), t
        live, assigned = dev.policies()
        assert np.array_equal(live, first if t < STEPS - 1 else then), t
        assert np.array_equal(assigned, first if t < 10 else then), t
    assert np.array_equal(dev.rng_state(), ora.rng_state())
    for e in range(n):
        a, b = dev.get_state(e), ora.get_state(e)
        assert np.array_equal(a, b), (e, np.nonzero(a != b)[0][:12].tolist())
    dev.close(), ora.close()


# ---------------------------------------------------------------------------------------------------------------- 8. copies, faults, refusals
def test_clones_carry_live_classes_and_assignments(monkeypatch):
    """A clone copies the hot row whole: live classes and assignment of the source; the destination regenerates into the assignment it received.
    cc4_get_state / cc4_set_state carry both into a second handle of another default configuration."""
    n = 8
    a = _env(n, steps=STEPS, rng_mode=1, autoreset=True)
    a.set_policies(red=[3, 2, 1, 0, M.KEEP, M.KEEP, M.KEEP, M.KEEP], green=[1, 0, 1, 0] + [M.KEEP] * 4, blue=[0, 1, 1, 0] + [M.KEEP] * 4)
    a.reset(seeds=40)
    a.set_policies(red=[M.KEEP, 0, M.KEEP, M.KEEP] + [M.KEEP] * 4)      # episode 1: live (2, 0, 1), assigned (0, 0, 1) from now on
    a.clone_episodes(np.array([0, 1, 2]), np.array([4, 5, 6]))
    live, assigned = a.policies()
    assert live[[4, 5, 6]].tolist() == [[3, 1, 0], [2, 0, 1], [1, 1, 1]] and assigned[[4, 5, 6]].tolist() == [[3, 1, 0], [0, 0, 1], [1, 1, 1]]
    assert live[7].tolist() == [0, 0, 0] and assigned[7].tolist() == [M.DEFAULT] * 3
    b = _twin(monkeypatch, n, steps=STEPS, rng_mode=1, autoreset=True, red_policy=1)
    b.reset(seeds=41)
    b.restore(3, a.snapshot(5))
    assert b.policies()[0][3].tolist() == [2, 0, 1] and b.policies()[1][3].tolist() == [0, 0, 1]
    for t in range(STEPS + 2):                                         # across the regeneration of call 30
        act = random_actions(9, t, n)
        act_b = act.copy()
        act_b[3] = act[5]                                              # (the episode that moved takes the same actions on both handles)
        a.step(act), b.step(act_b)
    live, assigned = a.policies()
    assert live[[4, 5, 6, 7]].tolist() == [[3, 1, 0], [0, 0, 1], [1, 1, 1], [0, 0, 0]] and np.array_equal(live[:3], live[4:7])
    lb, ab = b.policies()
    assert lb[3].tolist() == [0, 0, 1] and ab[3].tolist() == [0, 0, 1] and (lb[[0, 1, 2]] == [1, 0, 0]).all()
    assert np.array_equal(a.get_state(5), b.get_state(3))             # the same episode on both handles, regeneration included
    a.close(), b.close()


def test_out_of_range_classes_are_skipped_and_reported():
    from cage_challenge_4_amd.vec_env import CC4EngineError
    n = 70
    env = _env(n, steps=STEPS, rng_mode=1)
    env.set_policies(red=1, green=0, blue=1)
    env.reset(seeds=3)
    red = np.full(n, 2, np.int8)
    green = np.full(n, M.KEEP, np.int8)
    bad = {3: (4, M.KEEP), 17: (2, 2), 64: (-3, M.KEEP), 69: (M.DEFAULT, 1)}
    for e, (r, g) in bad.items():
        red[e], green[e] = r, g
    with pytest.raises(CC4EngineError, match='INDEX_OUT_OF_RANGE'):
        env.set_policies(red=red, green=green)
    live, assigned = env.policies()
    assert (live == [1, 0, 1]).all()
    for e in range(n):
        assert assigned[e].tolist() == ([1, 0, 1] if e in bad else [2, 0, 1]), e
    env.set_policies(red=M.DEFAULT)                                    # a clean call raises nothing: the fault word was cleared
    assert (env.policies()[1] == M.DEFAULT).all()
    with pytest.raises(ValueError):
        env.set_policies(red=np.zeros(n + 1, np.int8))
    env.close()


def test_device_calls_are_refused_inside_a_rollout():
    env = _env(8192, steps=50, rng_mode=1)
    env.reset(seeds=4)
    lib, h = env.lib, env._h
    K = 4
    assert env.run_kernel_for(20) == 'k_run_philox1'
    assert lib.cc4_rollout_begin(h, K) == 0, lib.cc4_last_error(h)
    host = np.zeros(3 * 8192, np.int8)
    p = host.ctypes.data_as(ctypes.c_void_p)
    for rc in (lib.cc4_set_policies_device(h, p, None, None), lib.cc4_policies_device(h, p, None), lib.cc4_reset_device(h, None, None),
               lib.cc4_set_policies(h, p, None, None), lib.cc4_get_policies(h, p, None)):
        assert rc == -2 and b'rollout' in lib.cc4_last_error(h)
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
    env.set_policies(red=2)                                            # after the rollout: fine
    assert (env.policies()[1][:, 0] == 2).all()
    env.close()
