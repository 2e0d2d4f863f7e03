"""GPU: device-resident action plans (cc4_run_plan_device / CC4VecEnv.run_plan).  Every comparison is exact.
1. the persistent plan kernels against the trajectories recorded from the reference, at full batch (every episode a copy of a fixture);
2. a plan == the same rows through k single steps on a twin handle, for every kernel cc4_plan_kernel_for can name;
3. a plan of the stand-in policy's draws == cc4_run_random_steps;
4. plan calls between the other ways of stepping one handle;
5. the self-check (CC4_PERSIST_VERIFY=1) counts plan calls and finds no disagreement;
7. refusals."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

import golden_util as G
from oracle_binding import random_actions
from plan_util import random_plan, run_plan, same_handles, single_steps

pytestmark = pytest.mark.gpu
CHUNK = 64          # steps per run_plan call of the reference-anchored tests (the recorded observations of 8192 episodes stay within ~300 MB)


def _env(n, **kw):
    from cage_challenge_4_amd import CC4VecEnv
    kw.setdefault('strict', False)
    return CC4VecEnv(n, **kw)


def _twin(monkeypatch, n, **kw):
    """A second device handle on ONE stream (CC4_GROUPS=1) and without a self-check shadow: the runtime maps streams onto 16 hardware queues, and a
    rollout's policy streams must not come to share the queue its persistent kernel occupies (conftest.py) -- two full handles, their shadows and
    four policy streams are more than 16."""
    monkeypatch.setenv('CC4_GROUPS', '1')
    monkeypatch.setenv('CC4_PERSIST_VERIFY_EVERY', '0')
    try:
        return _env(n, **kw)
    finally:
        monkeypatch.delenv('CC4_GROUPS')
        monkeypatch.delenv('CC4_PERSIST_VERIFY_EVERY')


def _first_bad(got, want):
    bad = np.argwhere(np.asarray(got) != np.asarray(want))
    return bad[0].tolist() if bad.size else None


# ---------------------------------------------------------------------------------------------------------------- 1. reference-anchored
@pytest.mark.parametrize('steps,n', [(200, 6656), (500, 8192), (1000, 6656)])
def test_persistent_plan_kernel_matches_reference_counter_mode(steps, n):
    """The ctrstep_* episodes of one length, started as golden_util.ctr_start starts them, in a batch the persistent kernel serves: episode i is a
    copy of fixture i mod F and runs fixture i mod F's recorded actions and messages; rewards, dones and observations of every episode at every
    step equal the arrays recorded from the reference."""
    from cage_challenge_4_amd import CC4VecEnv
    fixes = [f for f in map(G.load_ctr, G.list_ctr_fixtures()) if f['steps'] == steps]
    assert fixes, 'no counter-mode fixture of this length'
    F = len(fixes)
    env = _env(n, steps=steps, rng_mode=1)
    env.reset(seeds=1)
    for i, f in enumerate(fixes):
        g = CC4VecEnv(1, steps=steps, rng_mode=0, red_policy=f['red_policy'], green_policy=f['green_policy'], blue_policy=f['blue_policy'])
        g.reset(seeds=np.array([f['seed']], np.uint64))
        assert np.array_equal(g.reset(seeds=None)[0], f['obs'][0]), f['name']
        env.restore(i, g.snapshot(0))
        g.close()
    idx = np.arange(n) % F
    env.clone_episodes(idx[F:], np.arange(F, n))
    env.set_seed(np.array([fixes[i]['key'] for i in idx], np.uint64))
    T = min(f['actions'].shape[0] for f in fixes)
    assert T == steps
    zero = np.zeros((T, 5, 8), np.uint8)
    for t0 in range(0, T, CHUNK):
        t1 = min(T, t0 + CHUNK)
        k = t1 - t0
        assert env.plan_kernel_for(k) == ('k_run_philox1p' if k >= 10 else 'k_step_philox1')
        plan = np.stack([f['actions'][t0:t1] for f in fixes], 1)[:, idx]
        msgs = np.stack([(f['messages'] if f['messages'] is not None else zero)[t0:t1] for f in fixes], 1)[:, idx]
        obs, rew, done, info = env.run_plan(plan, msgs, record_obs=True)
        assert not info['err'].any()
        want = np.stack([f['reward'][t0:t1] for f in fixes], 1)[:, idx]
        assert _first_bad(rew, want) is None, ('reward [step, episode]', t0, _first_bad(rew, want))
        want = np.stack([f['done'][t0:t1] for f in fixes], 1)[:, idx]
        assert _first_bad(done, want) is None, ('done [step, episode]', t0, _first_bad(done, want))
        want = np.stack([f['obs'][t0 + 1:t1 + 1] for f in fixes], 1).astype(np.uint8)
        seq = info['obs_seq']
        for fi in range(F):          # (fixture by fixture: no [k, n, 578] array of expected values)
            got = seq[:, fi::F]
            assert np.array_equal(got, np.broadcast_to(want[:, fi:fi + 1], got.shape)), (fixes[fi]['name'], t0, _first_bad(got, want[:, fi:fi + 1]))
        assert np.array_equal(obs, seq[-1])
    env.close()


def test_persistent_plan_kernel_matches_reference_numpy_stream():
    """The same with the 500-step default-policy traj_* episodes on the numpy stream (k_run_pcgp), seeded as
    test_hip_matches_reference_golden_trajectories seeds them, including the PCG64 stream position after the last step."""
    fixes = [f for f in map(G.load, G.list_fixtures()) if f['steps'] == 500 and not (f['red_policy'] or f['green_policy'] or f['blue_policy'])]
    assert len(fixes) >= 3
    n, F = 8192, len(fixes)
    idx = np.arange(n) % F
    env = _env(n, steps=500)
    env.reset(seeds=np.array([fixes[i]['seed'] for i in idx], np.uint64))
    ctor = np.array([fixes[i]['reset_seed'] < 0 for i in idx], np.uint8)
    env.reset(seeds=None, env_mask=ctor)
    obs = env.reset(seeds=np.array([max(fixes[i]['reset_seed'], 0) for i in idx], np.uint64), env_mask=1 - ctor)
    assert np.array_equal(obs, np.stack([f['obs'][0] for f in fixes])[idx])
    T = min(f['actions'].shape[0] for f in fixes)
    zero = np.zeros((T, 5, 8), np.uint8)
    for t0 in range(0, T, CHUNK):
        t1 = min(T, t0 + CHUNK)
        k = t1 - t0
        assert env.plan_kernel_for(k) == ('k_run_pcgp' if k >= 10 else 'k_step')
        plan = np.stack([f['actions'][t0:t1] for f in fixes], 1)[:, idx]
        msgs = np.stack([(f['messages'] if f['messages'] is not None else zero)[t0:t1] for f in fixes], 1)[:, idx]
        obs, rew, done, info = env.run_plan(plan, msgs, record_obs=True)
        assert not info['err'].any()
        assert np.array_equal(rew, np.stack([f['reward'][t0:t1] for f in fixes], 1)[:, idx]), t0
        assert np.array_equal(done, np.stack([f['done'][t0:t1] for f in fixes], 1)[:, idx]), t0
        want = np.stack([f['obs'][t0 + 1:t1 + 1] for f in fixes], 1).astype(np.uint8)
        seq = info['obs_seq']
        for fi in range(F):
            got = seq[:, fi::F]
            assert np.array_equal(got, np.broadcast_to(want[:, fi:fi + 1], got.shape)), (fixes[fi]['name'], t0)
    st = env.rng_state()
    bad = [i for i in range(n) if not G.rng_words_match(fixes[idx[i]]['rng'][T], st[i])]
    assert not bad, bad[:8]
    env.close()


# ---------------------------------------------------------------------------------------------------------------- 2. plan == k single steps
CASES = [  # batch, rng_mode, CC4_PHILOX_LEAN, event log, the kernel cc4_plan_kernel_for names for 170 steps
    (8192, 1, None, False, 'k_run_philox1p'), (6656, 0, None, False, 'k_run_pcgp'),
    (1024, 1, '0', False, 'k_step_philox'), (1024, 1, '1', False, 'k_step_philox1'), (64, 0, None, False, 'k_step'),
    (8192, 1, None, True, 'k_step_philox1')]


@pytest.mark.parametrize('autoreset', [True, False])
@pytest.mark.parametrize('with_msgs', [False, True])
@pytest.mark.parametrize('case', CASES, ids=lambda c: f'{c[0]}-{c[4]}' + ('-evlog' if c[3] else ''))
def test_plan_equals_single_steps(case, with_msgs, autoreset, monkeypatch):
    """170 rows of random indices over the full ranges (negative and out-of-list ones included) on 150-step episodes: with autoreset the plan
    crosses the episodes' ends and regenerates them, without it runs past them (E_STEP_PAST_END).  A twin handle takes the same rows through
    170 calls of step()."""
    n, mode, lean, evlog, kernel = case
    if lean is not None:
        monkeypatch.setenv('CC4_PHILOX_LEAN', lean)
    a = _env(n, steps=150, rng_mode=mode, autoreset=autoreset)
    b = _env(n, steps=150, rng_mode=mode, autoreset=autoreset)
    for e in (a, b):
        e.reset(seeds=900 + n)
        if evlog:
            e.enable_event_log()
    k = 170
    assert a.plan_kernel_for(k) == kernel
    plan, msgs = random_plan(np.random.default_rng(n + 2 * mode + with_msgs), k, n, with_msgs)
    obs, rew, done, info = run_plan(a, plan, msgs)
    err = info['err'].copy()
    o2, r2, d2, e2 = single_steps(b, plan, msgs)
    assert np.array_equal(rew, r2), _first_bad(rew, r2)
    assert np.array_equal(done, d2), _first_bad(done, d2)
    assert np.array_equal(info['obs_seq'], o2), _first_bad(info['obs_seq'], o2)
    assert np.array_equal(obs, o2[-1])
    assert np.array_equal(err, e2), _first_bad(err, e2)          # every flag some step raised, as the k single calls showed them
    assert (err & (1 << 7)).any() == (not autoreset)
    assert same_handles(a, b, sample=(0, 1, n // 2, n - 1)) is None
    assert np.array_equal(a.device_actions(), plan[-1])
    a.close(), b.close()


# ---------------------------------------------------------------------------------------------------------------- 3. the stand-in's draws
@pytest.mark.parametrize('mode', [1, 0])
def test_plan_of_the_stand_in_draws_equals_run_random_steps(mode):
    n, k, seed0, t0 = 8192, 40, 77, 5
    a = _env(n, steps=100, rng_mode=mode, autoreset=True)
    b = _env(n, steps=100, rng_mode=mode, autoreset=True)
    a.reset(seeds=31), b.reset(seeds=31)
    plan = np.zeros((k, n, 5), np.int32)
    for j in range(k):
        a._chk(a.lib.cc4_random_actions_device(a._h, ctypes.c_uint64(seed0), ctypes.c_uint32(t0 + j)), 'cc4_random_actions_device')
        plan[j] = a.device_actions()
    assert np.array_equal(plan[3], random_actions(seed0, t0 + 3, n))
    assert a.plan_kernel_for(k).startswith('k_run_') and b.run_kernel_for(k).startswith('k_run_')
    a.run_plan(plan)
    b.run_random_steps(seed0, t0, k, timed=False)
    assert same_handles(a, b) is None
    assert np.array_equal(a.err, b.err)
    a.close(), b.close()


# ---------------------------------------------------------------------------------------------------------------- 4. call sequences
@pytest.mark.parametrize('n,mode', [(6656, 1), (8192, 0)])
def test_plan_calls_between_the_other_ways_of_stepping(n, mode, monkeypatch):
    """Plan calls alternate with run_random_steps, single steps, rollouts (counter mode), clones and masked resets on one handle -- ticket parity and
    the progress words' base are bookkeeping all one-launch forms share; the twin only ever takes single steps.  k = 1, persist_min_k - 1,
    persist_min_k, runs of four with single steps behind, runs of eight with a ragged tail."""
    a = _env(n, steps=55, rng_mode=mode, autoreset=True)
    b = _twin(monkeypatch, n, steps=55, rng_mode=mode, autoreset=True)
    a.reset(seeds=4000 + n), b.reset(seeds=4000 + n)
    rng = np.random.default_rng(n)
    one = a.plan_kernel_for(10)
    assert one == ('k_run_philox1p' if mode else 'k_run_pcgp') and a.plan_kernel_for(9) == a.step_kernel
    seq = [('plan', 1), ('plan', 9), ('random', 10), ('plan', 10), ('rollout', 12), ('plan', 37), ('clone', 0), ('plan', 77), ('step', 1),
           ('reset', 0), ('plan', 10), ('random', 13), ('plan', 11), ('rollout', 9), ('plan', 16)]
    t = 0
    for i, (kind, k) in enumerate(seq):
        if kind == 'rollout' and not mode:
            continue
        if kind == 'plan':
            plan, msgs = random_plan(rng, k, n, messages=bool(i % 2))
            obs, rew, done, info = a.run_plan(plan, msgs, record_obs=True)
            o2, r2, d2, e2 = single_steps(b, plan, msgs)
            assert np.array_equal(rew, r2) and np.array_equal(done, d2) and np.array_equal(info['obs_seq'], o2), (i, kind, k)
            assert np.array_equal(info['err'], e2), (i, kind, k)
        elif kind in ('random', 'rollout'):
            if kind == 'random':
                a.run_random_steps(7 + i, t, k, timed=False)
            else:
                a.run_rollout(k, 'random', 7 + i, t)
            for j in range(k):
                b.step(random_actions(7 + i, t + j, n))
            t += k
        elif kind == 'step':
            act = random_plan(rng, 1, n)[0][0]
            a.step(act), b.step(act)
        elif kind == 'clone':
            src, dst = np.arange(0, 64), np.arange(n - 64, n)
            a.clone_episodes(src, dst), b.clone_episodes(src, dst)
        else:
            mask = (np.arange(n) % 3 == 0).astype(np.uint8)
            seeds = np.arange(n, dtype=np.uint64) + 99
            a.reset(seeds=seeds, env_mask=mask), b.reset(seeds=seeds, env_mask=mask)
        what = same_handles(a, b) if (i % 4 == 3 or i == len(seq) - 1) else None
        assert what is None, (i, kind, k, what)
        a._fetch(), b._fetch()
        assert np.array_equal(a._obs, b._obs) and np.array_equal(a._rew, b._rew) and np.array_equal(a._done, b._done), (i, kind, k)
    a.close(), b.close()


# ---------------------------------------------------------------------------------------------------------------- 5. the self-check
_VERIFY_CHILD = r'''
import sys
import numpy as np
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, sys.argv[1] + '/tests')
from cage_challenge_4_amd import CC4VecEnv
from plan_util import random_plan
for n, mode in ((8192, 1), (6656, 0)):
    env = CC4VecEnv(n, steps=40, rng_mode=mode, autoreset=True, strict=False)
    env.reset(seeds=12)
    rng = np.random.default_rng(n)
    calls = 0
    for k, rec, m in ((12, True, True), (45, False, False), (10, True, False), (70, True, True)):
        plan, msgs = random_plan(rng, k, n, m)
        assert env.plan_kernel_for(k).startswith('k_run_')
        env.run_plan(plan, msgs, record_obs=rec)
        calls += 1
    env.run_plan(random_plan(rng, 3, n)[0])            # (per-step form: nothing to check)
    print('VERIFY', n, mode, calls, *env.verify_stats())
    env.close()
'''


def test_self_check_counts_plan_calls_and_agrees():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, CC4_PERSIST_VERIFY='1')
    pr = subprocess.run([sys.executable, '-c', _VERIFY_CHILD, root], env=env, capture_output=True, text=True, timeout=600)
    assert pr.returncode == 0, pr.stdout[-2000:] + pr.stderr[-4000:]
    rows = [ln.split() for ln in pr.stdout.splitlines() if ln.startswith('VERIFY')]
    assert len(rows) == 2, pr.stdout
    for _, n, mode, calls, checked, bad in rows:
        assert int(checked) == int(calls) and int(bad) == 0, (n, mode, calls, checked, bad)
    # the sampled default check (every CC4_PERSIST_VERIFY_EVERY-th persistent call, 1024 unless set) counts plan calls too
    env = dict(os.environ, CC4_PERSIST_VERIFY_EVERY='2')
    env.pop('CC4_PERSIST_VERIFY', None)
    pr = subprocess.run([sys.executable, '-c', _VERIFY_CHILD, root], env=env, capture_output=True, text=True, timeout=600)
    assert pr.returncode == 0, pr.stdout[-2000:] + pr.stderr[-4000:]
    rows = [ln.split() for ln in pr.stdout.splitlines() if ln.startswith('VERIFY')]
    assert len(rows) == 2, pr.stdout
    for _, n, mode, calls, checked, bad in rows:
        assert int(checked) == int(calls) // 2 and int(bad) == 0, (n, mode, calls, checked, bad)


# ---------------------------------------------------------------------------------------------------------------- 7. refusals
def test_refusals_enqueue_nothing(monkeypatch):
    from cage_challenge_4_amd._lib import CC4Error
    n = 6656
    a = _env(n, steps=60, rng_mode=1, autoreset=True)
    b = _twin(monkeypatch, n, steps=60, rng_mode=1, autoreset=True)
    a.reset(seeds=3), b.reset(seeds=3)
    lib, h = a.lib, a._h
    rng = np.random.default_rng(1)
    plan = random_plan(rng, 12, n)[0]
    with pytest.raises(ValueError):
        a.run_plan(plan[:0])
    p = ctypes.c_void_p()
    a._chk(lib.cc4_actions_device(h, ctypes.byref(p)), 'cc4_actions_device')
    assert lib.cc4_run_plan_device(h, 0, p, None, None, None, None) == -2 and lib.cc4_run_plan_device(h, -3, p, None, None, None, None) == -2
    assert lib.cc4_run_plan_device(h, 1, None, None, None, None, None) == -2
    a._chk(lib.cc4_rollout_begin(h, 10), 'cc4_rollout_begin')              # a rollout in flight
    assert lib.cc4_run_plan_device(h, 1, p, None, None, None, None) == -2 and b'rollout' in lib.cc4_last_error(h)
    assert a.plan_kernel_for(12) == a.step_kernel
    G_, blk = ctypes.c_int32(), ctypes.c_int32()
    rc = lib.cc4_rollout_groups(h, ctypes.byref(G_), ctypes.byref(blk))
    for j in range(10):
        for g in range(G_.value):
            rc = rc or lib.cc4_rollout_sync(h, g if j > 0 else -1, j - 1, g, j, None)
            rc = rc or lib.cc4_rollout_random_policy(h, g, j, ctypes.c_uint64(4), ctypes.c_uint32(j), None)
    for g in range(G_.value):
        rc = rc or lib.cc4_rollout_sync(h, g, 9, -1, 0, None)
    assert lib.cc4_rollout_end(h) == 0 and rc == 0, lib.cc4_last_error(h)
    for j in range(10):
        b.step(random_actions(4, j, n))
    # nothing of the refused calls reached the device: the handle steps on as its twin does
    obs, rew, done, info = a.run_plan(plan)
    o2, r2, d2, e2 = single_steps(b, plan)
    assert np.array_equal(rew, r2) and np.array_equal(done, d2) and same_handles(a, b) is None
    a.close(), b.close()
    one = _env(4, steps=50, rng_mode=1)
    one.reset(seeds=5)
    os.environ.setdefault('NCCL_SOCKET_IFNAME', 'lo')
    ident = (ctypes.c_uint8 * 128)()
    assert one.lib.cc4_comm_unique_id(ident) == 0
    one._chk(one.lib.cc4_comm_init(one._h, 0, 1, ident), 'cc4_comm_init')
    with pytest.raises(CC4Error, match='communicator'):
        one.run_plan(np.zeros((2, 4, 5), np.int32))
    assert one.plan_kernel_for(2) == one.step_kernel
    one.step(np.zeros((4, 5), np.int32))
    one.close()
