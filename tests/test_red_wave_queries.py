"""GPU: the one-wave counter-mode kernels answer what each side-by-side red action first reads from its agent's session list (its
session by id, the agent's sessions on the target host) for all six agents in one pass of the wave (rs_wave_query: eight list
entries per round, further rounds for longer lists).  The scenario rarely gives an agent more than a handful of sessions, so these
tests add them by hand -- past 8 and past 32 for some agents, so that the second and the fifth round run -- and compare every step
with the CPU oracle, on k_step_philox1 (full build, with submitted red actions that name those sessions and hosts) and on the
persistent k_run_philox1 and the fast build of k_step_philox1 (seeded random blue actions)."""
import json
import numpy as np
import pytest
import ext_util as X
from oracle_binding import OracleVecEnv, random_actions

pytestmark = pytest.mark.gpu

SE_ADD_RED_SESSION, SE_SET_RED_ACTIVE = 5, 9
EXTRA = (36, 9, 12, 0, 17, 9)          # sessions added per red agent: agent 0 past 32, agent 4 past 16, most past 8, one untouched


def _dev(n, **kw):
    from cage_challenge_4_amd import CC4VecEnv
    return CC4VecEnv(n, **kw)


def _add_sessions(ora, e, salt):
    """Adds EXTRA[r] sessions to agent r of the oracle's episode e (abstract or not, root or not, spread over the hosts) and makes
    every agent that has sessions active.  Returns the number of sessions added."""
    d = json.loads(ora.true_state_json(e))
    hosts = [h['h'] for h in d['hosts']]
    added = 0
    for r, k in enumerate(EXTRA):
        for j in range(k):
            h = hosts[(7 * r + 3 * j + salt) % len(hosts)]
            flags = (4 if (j + r) % 3 else 0) | (1 if j % 4 == 1 else 0) | (2 if j % 5 == 2 else 0)
            if ora.edit_state(e, SE_ADD_RED_SESSION, r, h, flags) >= 0:
                added += 1
        if k:
            ora.edit_state(e, SE_SET_RED_ACTIVE, r, 1)
    return added


def _max_sessions(ora, e):
    d = json.loads(ora.true_state_json(e))
    return max(len(a['sessions']) for a in d['red'])


def test_submitted_red_actions_on_long_session_lists_match_oracle(monkeypatch):
    """k_step_philox1 (full build, cc4_step_ex): submitted red actions naming sessions and hosts of long lists, every step against
    the oracle, the packed state and the cold rows at the end."""
    monkeypatch.setenv('CC4_PHILOX_LEAN', '1')
    n, steps, T = 40, 100, 60
    dev = _dev(n, steps=steps, rng_mode=1, strict=False)
    assert dev.step_kernel == 'k_step_philox1'
    ora = OracleVecEnv(n, steps=steps, rng_mode=1)
    assert np.array_equal(dev.reset(seeds=2024), ora.reset(seeds=2024))
    for e in range(n):
        assert _add_sessions(ora, e, e) > 40
        dev.restore(e, ora.snapshot(e))
    assert _max_sessions(ora, 0) > 32
    rng = np.random.default_rng(5)
    red, green = dev.agent_actions('red'), dev.agent_actions('green')
    for t in range(T):
        X.random_ext([ora.true_state_json(e) for e in range(n)], rng, 0.7, 0.05, red, green)
        acts = random_actions(2024, t, n)
        if t % 5 == 2:
            d = dev.step(acts); o = ora.step_ex(acts, None, None, None)
        else:
            d = dev.step_ex(acts, None, red, green); o = ora.step_ex(acts, None, red, green)
        bad = np.nonzero((d[0] != o[0]).any(axis=1) | (d[1] != o[1]) | (d[2] != o[2]) | (d[3]['err'] != o[3]['err']))[0]
        assert bad.size == 0, (t, bad[:10].tolist())
    for e in range(n):
        (h1, c1), (h2, c2) = dev.snapshot(e), ora.snapshot(e)
        assert np.array_equal(h1, h2), f'packed state differs env {e} at byte offsets {np.nonzero(h1 != h2)[0][:20].tolist()}'
        assert np.array_equal(c1, c2), f'cold row differs env {e}'
    dev.close(); ora.close()


def test_long_session_lists_on_the_persistent_and_the_step_kernel_match_oracle():
    """The bench's own path: k_run_philox1 (calls of 10 steps and more) and the fast k_step_philox1 (shorter calls) on a batch in which
    every eighth episode carries long session lists; outputs after every call, every hot row at the end."""
    n, steps, seed0 = 6656, 200, 808
    dev = _dev(n, steps=steps, rng_mode=1, autoreset=True, strict=False)
    assert dev.run_kernel_for(10) == 'k_run_philox1' and dev.run_kernel_for(9) == 'k_step_philox1'
    ora = OracleVecEnv(n, steps=steps, rng_mode=1, autoreset=True)
    assert np.array_equal(dev.reset(seeds=seed0), ora.reset_batch(seed0))
    edited = list(range(0, n, 8))
    for e in edited:
        _add_sessions(ora, e, e)
        dev.restore(e, ora.snapshot(e))
    assert _max_sessions(ora, 0) > 32
    t = 0
    for K in (10, 3, 25, 1, 12, 5, 40, 10):
        dev.run_random_steps(seed0, t, K, timed=False)
        for k in range(K):
            o = ora.step_batch(random_actions(seed0, t + k, n))
        t += K
        dev.synchronize(); dev._fetch()
        bad = np.nonzero((dev._obs != o[0]).any(axis=1) | (dev._rew != o[1]) | (dev._done.astype(bool) != o[2]) | (dev._err != o[3]['err']))[0]
        assert bad.size == 0, (K, t, bad[:10].tolist())
    assert max(_max_sessions(ora, e) for e in edited[:16]) > 32
    rows = dev.get_states()
    bad = [e for e in range(n) if not np.array_equal(rows[e], ora.get_state(e))]
    assert not bad, bad[:10]
    dev.close(); ora.close()
