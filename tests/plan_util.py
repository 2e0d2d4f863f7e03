"""Helpers of the plan tests (tests/test_plan*.py): random plans over the full index ranges, and a twin handle stepped one call at a time."""
import numpy as np

ACT_LEN = (82, 82, 82, 82, 242)


def random_plan(rng, k, n, messages=False):
    """[k, n, 5] wrapper indices over each agent's full range and beyond: negative (no action) and past the end of the list (Sleep) included;
    optionally [k, n, 5, 8] message bits."""
    a = np.stack([rng.integers(-4, ACT_LEN[b] + 8, size=(k, n)) for b in range(5)], axis=2).astype(np.int32)
    m = rng.integers(0, 2, size=(k, n, 5, 8)).astype(np.uint8) if messages else None
    return a, m


def single_steps(env, plan, msgs=None):
    """The plan through k calls of env.step (strict=False): (obs_seq uint8 [k, n, 578], rewards [k, n], dones [k, n], err_or [n])."""
    k, n = plan.shape[:2]
    obs = np.zeros((k, n, 578), np.uint8)
    rew = np.zeros((k, n), np.float32)
    done = np.zeros((k, n), bool)
    err = np.zeros(n, np.uint32)
    for j in range(k):
        try:
            env.step(plan[j], None if msgs is None else msgs[j])
        except ValueError:          # a step past the episode's end (autoreset off): the outputs were fetched before the flag raised
            pass
        obs[j], rew[j], done[j] = env._obs, env._rew, env._done.astype(bool)
        err |= env._err
    return obs, rew, done, err


def run_plan(env, plan, msgs=None, record_obs=True):
    """env.run_plan, with the outputs of a plan that ran past an episode's end (ValueError, as step()) taken from the exception."""
    try:
        return env.run_plan(plan, msgs, record_obs=record_obs)
    except ValueError as e:
        return e.plan_outputs


def same_handles(a, b, sample=(0, 1, 7)):
    """None if two handles stand at the same point -- outputs, generator positions, every hot row, the true state of a sample of episodes, last
    actions -- else what differs."""
    a.synchronize(), b.synchronize()
    for e in (a, b):              # (not _fetch: a step past an episode's end would raise here)
        e._chk(e.lib.cc4_fetch(e._h, *e._p_out), 'cc4_fetch')
    for what, x, y in (('observations', a._obs, b._obs), ('reward', a._rew, b._rew), ('done', a._done, b._done),
                       ('generator state', a.rng_state(), b.rng_state()), ('hot rows', a.get_states(), b.get_states()),
                       ('device actions', a.device_actions(), b.device_actions())):
        if not np.array_equal(x, y):
            bad = np.nonzero((np.asarray(x).reshape(a.num_envs, -1) != np.asarray(y).reshape(a.num_envs, -1)).any(axis=1))[0]
            return f'{what} differ: first episodes {bad[:8].tolist()} of {bad.size}'
    for i in sample:
        if i < a.num_envs and a.true_state_json(i) != b.true_state_json(i):
            return f'true state of episode {i} differs'
    return None
