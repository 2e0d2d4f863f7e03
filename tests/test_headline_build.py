"""GPU: the headline build of the persistent kernel (k_run_philox1: persist_loop<.., HEAD>) against the CPU oracle.

The build is compiled for ONE shape of call -- the blue actions drawn in the kernel, no actions or messages given (persist_launch's head_shape decides;
any other call takes k_run_philox1g or the plan / per-step kernels).  So, after every call: every hot row, the generator states, rewards, dones, error
words, the int32 observations, the actions the last step drew, and sampled cold rows (handover_util.fetch_final / first_mismatch; the cells' seeds:
RESET_SEED, RANDOM_SEED0, RANDOM_T0).
 (a) 6656 episodes of 40 steps, calls of 12, 45 and 70 steps -- the 45-step call regenerates on the last step of a run of 4, the 70-step call twice
     strictly inside a run of 8 (asserted from the oracle's done rows) -- every call under the self-check (CC4_PERSIST_VERIFY=1): the shadow's per-step
     launches must agree too;
 (b) 7001 episodes -- odd and no multiple of 256: the byte arrays end unaligned and the partitions are uneven -- calls of 10 (the shortest persistent
     call) and 23 steps;
 (c) one handle stepped in turn by cc4_run_random_steps, by a step with the host's actions and messages, and by a plan call with messages: a call that
     carries actions or messages must never reach the specialised kernel -- it would ignore them, and every row would leave the oracle's."""
import numpy as np
import pytest

import handover_util as H
from oracle_binding import OracleVecEnv, random_actions
from plan_util import random_plan

pytestmark = pytest.mark.gpu


def _snapshot(ora, n, regen, actions, o, r, d, err):
    t = H.Trajectory()
    t.regen, t.actions = regen, np.asarray(actions, np.int32)
    t.obs_packed = t.rewards = t.dones = None          # (cc4_run_random_steps records no rows: the call's end is what is compared)
    t.obs_last, t.reward_last, t.done_last, t.err_last = o.copy(), r.copy(), d.copy(), err.copy()
    t.hot = np.stack([ora.get_state(e) for e in range(n)])
    t.cold = {e: ora.get_cold(e) for e in sorted(set(range(0, n, H.COLD_STRIDE)) | {n - 1})}
    t.rng = ora.rng_state()
    return t


def _oracle_random_calls(n, steps, calls):
    """The oracle stepped through consecutive cc4_run_random_steps calls of `calls` steps; one snapshot behind each (regen [k, n]: the steps that re-create)."""
    ora = OracleVecEnv(n, steps=steps, rng_mode=1, autoreset=True)
    ora.reset_batch(H.RESET_SEED)
    t, out = H.RANDOM_T0, []
    for k in calls:
        regen = np.zeros((k, n), bool)
        for j in range(k):
            regen[j] = ora._done
            a = random_actions(H.RANDOM_SEED0, t + j, n)
            o, r, d, info = ora.step_batch(a)
        t += k
        out.append(_snapshot(ora, n, regen, a, o, r, d, info['err']))
    ora.close()
    return out


def _compare(env, snap, what):
    final = H.fetch_final(env.lib, env._h, snap, plan=False)
    final['last actions drawn'] = (env.device_actions(), snap.actions)
    bad = H.first_mismatch(None, snap, final=final)
    assert bad is None, f'{what}: {bad}'
    assert not snap.err_last.any(), what


def _regens_in_runs(n, steps, k, snap):
    """(step, run, position in the run, run length) of the call's regenerations, by the schedule's own run split."""
    cell = H.Cell('headline', n, 1, steps, (), H.Random(k), (), 1)
    return H.describe(cell, snap).regens


def _random_calls_against_oracle(n, steps, calls, verify):
    from cage_challenge_4_amd import CC4VecEnv
    snaps = _oracle_random_calls(n, steps, calls)
    env = CC4VecEnv(n, steps=steps, rng_mode=1, autoreset=True, strict=False)
    inside = []
    try:
        env.reset(seeds=H.RESET_SEED)
        t = H.RANDOM_T0
        for c, (k, snap) in enumerate(zip(calls, snaps)):
            assert env.run_kernel_for(k) == 'k_run_philox1', (n, k, env.run_kernel_for(k))
            env.run_random_steps(H.RANDOM_SEED0, t, k, timed=(c % 2 == 1))
            t += k
            _compare(env, snap, f'{n} episodes, call {c} of {k} steps')
            regens = _regens_in_runs(n, steps, k, snap)
            print(f'{n} episodes, call {c} of {k} steps: regenerations (step, run, q, run length) {regens}')
            inside += [g for g in regens if 0 < g[2] < g[3] - 1]
        stats = env.verify_stats()
        assert tuple(stats) == ((len(calls), 0) if verify else (0, 0)), stats
    finally:
        env.close()
    return inside


def test_headline_kernel_across_regenerations_under_the_self_check(monkeypatch):
    monkeypatch.setenv('CC4_PERSIST_VERIFY', '1')
    inside = _random_calls_against_oracle(6656, 40, (12, 45, 70), verify=True)
    assert inside, 'no call regenerated strictly inside a run: the sequence no longer covers a regeneration between two steps that keep the row in LDS'


def test_headline_kernel_on_an_odd_batch_and_the_shortest_call():
    # 15-step episodes: the 23-step call regenerates twice
    _random_calls_against_oracle(7001, 15, (10, 23), verify=False)


def test_calls_with_actions_or_messages_never_take_the_headline_kernel():
    from cage_challenge_4_amd import CC4VecEnv
    n, steps, K = 6656, 40, 12
    ora = OracleVecEnv(n, steps=steps, rng_mode=1, autoreset=True)
    env = CC4VecEnv(n, steps=steps, rng_mode=1, autoreset=True, strict=False)
    rng = np.random.default_rng(n)
    try:
        env.reset(seeds=H.RESET_SEED)
        ora.reset_batch(H.RESET_SEED)
        assert env.run_kernel_for(K) == 'k_run_philox1' and env.plan_kernel_for(K) == 'k_run_philox1p'
        t = H.RANDOM_T0
        for rnd in range(2):
            # the headline kernel
            regen = np.zeros((K, n), bool)
            for j in range(K):
                regen[j] = ora._done
                a = random_actions(H.RANDOM_SEED0, t + j, n)
                o, r, d, info = ora.step_batch(a)
            env.run_random_steps(H.RANDOM_SEED0, t, K, timed=False)
            t += K
            _compare(env, _snapshot(ora, n, regen, a, o, r, d, info['err']), f'round {rnd}: {K} random steps')
            # a step with the host's actions and messages
            act, msg = random_plan(rng, 1, n, True)
            got = env.step(act[0], msg[0])
            o, r, d, info = ora.step_batch(act[0], msg[0])
            assert np.array_equal(got[0], o) and np.array_equal(got[1], r) and np.array_equal(np.asarray(got[2], bool), np.asarray(d, bool)), f'round {rnd}: the host-action step'
            # a plan call with messages
            act, msg = random_plan(rng, K, n, True)
            rew, done = np.zeros((K, n), np.float32), np.zeros((K, n), bool)
            for j in range(K):
                o, r, d, info = ora.step_batch(act[j], msg[j])
                rew[j], done[j] = r, d
            obs, g_rew, g_done, g_info = env.run_plan(act, msg)
            assert np.array_equal(obs, o) and np.array_equal(g_rew.view(np.uint32), rew.view(np.uint32)) and np.array_equal(np.asarray(g_done, bool), done), f'round {rnd}: the plan call'
            assert np.array_equal(env.get_states(), np.stack([ora.get_state(e) for e in range(n)])), f'round {rnd}: hot rows behind the plan call'
            assert np.array_equal(env.rng_state(), ora.rng_state()), rnd
    finally:
        env.close()
        ora.close()
