"""The stand-in fixtures (tests/golden/ctrstand_*.npz, trajstand_*.npz; golden_util.load_standin) on a batch: reference episodes whose blue actions are
the draws cc4_run_random_steps makes inside the kernel.  In a batch stepped with `seed0` the episode in slot e draws from key seed0 + e, so the fixture
with action key akey replays in slot akey - seed0 of a batch of any size; everything else in the batch is an ordinary episode.

oracle_replay: every fixture of a mode once on the CPU oracle (shared by the tests of a session) -- its outputs of every step and its hot row after
every call of CALLS.  run_case: the fixtures placed in a device handle, the handle stepped through CALLS, every fixture's slot compared after every call
with the arrays recorded from the reference and with the oracle's hot row."""
import ctypes

import numpy as np

import golden_util as G
from mix_util import row_set
from oracle_binding import OracleVecEnv

CALLS = (1, 3, 9, 10, 12, 20, 45)            # steps per stepping call: 100 in all, one episode
ENDS = tuple(int(v) for v in np.cumsum(CALLS))
LONG = (10, 12, 20, 45)                      # the calls a one-launch kernel must have served (87 of the 100 steps)
STEPS = 100
ORDINARY_SEED = 7100                         # reset(seeds=) of the batch's other episodes

_fixtures, _replays = {}, {}


def fixtures(mode):
    """The stand-in fixtures of a mode (1: counter, 0: numpy stream), by offset d."""
    if mode not in _fixtures:
        fx = sorted((G.load_standin(p) for p in G.list_standin_fixtures(mode)), key=lambda f: f['d'])
        assert all(f['steps'] == STEPS and f['actions'].shape == (STEPS, 5) for f in fx)
        _fixtures[mode] = fx
    return _fixtures[mode]


def placement(mode, n, which):
    """(seed0, [(fixture, slot)]) -- 'low': seed0 = STANDIN_BASE, the fixtures sit at their offsets; 'high': the deepest fixture that fits sits in slot n - 1."""
    fx = fixtures(mode)
    fit = [f for f in fx if f['d'] < n]
    seed0 = G.STANDIN_BASE if which == 'low' else G.STANDIN_BASE + max(f['d'] for f in fit) - (n - 1)
    return seed0, [(f, f['akey'] - seed0) for f in fx if 0 <= f['akey'] - seed0 < n]


def _oracle_start(mode, fx):
    """One oracle episode per fixture at step 0: [(env, index)]; first observations and masks checked against the fixtures."""
    if mode == 1:
        env, obs0, masks = G.ctr_start(OracleVecEnv, fx)
        for i, f in enumerate(fx):
            assert np.array_equal(obs0[i], f['obs'][0]) and np.array_equal(masks[i], f['mask']), f['name']
        return [(env, i) for i in range(len(fx))]
    out = []
    for f in fx:
        assert f['reset_seed'] < 0          # CybORG(seed); wrapper.reset()
        env = OracleVecEnv(1, steps=STEPS, red_policy=f['red_policy'], green_policy=f['green_policy'], blue_policy=f['blue_policy'])
        env.reset(seeds=np.array([f['seed']], np.uint64))
        obs = env.reset(seeds=None)
        assert np.array_equal(obs[0], f['obs'][0]) and np.array_equal(env.mask()[0], f['mask']), f['name']
        out.append((env, 0))
    return out


def oracle_replay(mode):
    """{fixture name: {'obs' [101, 578], 'reward' [100], 'done' [100], 'err' [100], 'rng' [101, 7] (the generator's words), 'hot' {t: the hot row after t steps}}}
    of the oracle stepping each fixture's recorded actions.  Computed once per session."""
    if mode in _replays:
        return _replays[mode]
    fx = fixtures(mode)
    envs = _oracle_start(mode, fx)
    out = {}
    for f, (env, i) in zip(fx, envs):
        r = {'obs': np.zeros((STEPS + 1, 578), np.int32), 'reward': np.zeros(STEPS, np.float32), 'done': np.zeros(STEPS, bool),
             'err': np.zeros(STEPS, np.uint32), 'rng': np.zeros((STEPS + 1, 7), np.uint64), 'hot': {}}
        env._collect(i, reward=False)
        r['obs'][0] = env._obs[i]
        r['rng'][0] = env.rng_state()[i]
        for t in range(STEPS):
            a = np.ascontiguousarray(f['actions'][t], np.int32)
            env.lib.cc4o_step(env._h, i, a.ctypes.data_as(ctypes.c_void_p), None)
            env._collect(i)
            r['obs'][t + 1], r['reward'][t], r['done'][t], r['err'][t] = env._obs[i], env._rew[i], env._done[i], env._err[i]
            r['rng'][t + 1] = env.rng_state()[i]
            if t + 1 in ENDS:
                r['hot'][t + 1] = env.get_state(i)
        out[f['name']] = r
    for env in {id(e): e for e, _ in envs}.values():
        env.close()
    _replays[mode] = out
    return out


# ------------------------------------------------------------------------------------------------------------------------------------ device side
def start_device(mode, n, placed, **kw):
    """A device handle of n episodes: ordinary ones from reset(seeds=), and every (fixture, slot) of `placed` in its slot at step 0.
    Counter mode, as golden_util.ctr_start: a one-episode numpy-stream handle generates the fixture's scenario, a snapshot moves it over, cc4_set_seed
    puts the slot on the counter streams of the fixture's key.  Numpy stream: reset(seeds=) then reset(None) on the slot (CybORG(seed); wrapper.reset()),
    the classes per episode."""
    from cage_challenge_4_amd import CC4VecEnv
    seeds = np.uint64(ORDINARY_SEED) + np.arange(n, dtype=np.uint64)
    if mode == 1:
        env = CC4VecEnv(n, steps=STEPS, rng_mode=1, strict=False, **kw)
        env.reset(seeds=seeds)
        for f, slot in placed:
            g = CC4VecEnv(1, steps=STEPS, rng_mode=0, red_policy=f['red_policy'], green_policy=f['green_policy'], blue_policy=f['blue_policy'])
            g.reset(seeds=np.array([f['seed']], np.uint64))
            obs0 = g.reset(seeds=None)[0]
            assert np.array_equal(obs0, f['obs'][0]) and np.array_equal(g.action_mask[0], f['mask']), f['name']
            env.restore(slot, g.snapshot(0))
            g.close()
            seeds[slot] = f['key']
        env.set_seed(seeds)
        return env
    red, green, blue = (np.zeros(n, np.int8) for _ in range(3))
    mask = np.zeros(n, np.uint8)
    for f, slot in placed:
        assert f['reset_seed'] < 0
        red[slot], green[slot], blue[slot], seeds[slot], mask[slot] = f['red_policy'], f['green_policy'], f['blue_policy'], f['seed'], 1
    env = CC4VecEnv(n, steps=STEPS, rng_mode=0, strict=False, red_policy=red, green_policy=green, blue_policy=blue, **kw)
    env.reset(seeds=seeds)
    obs = env.reset(seeds=None, env_mask=mask)
    st = env.rng_state()
    for f, slot in placed:
        assert np.array_equal(obs[slot], f['obs'][0]) and np.array_equal(env.action_mask[slot], f['mask']), f['name']
        assert G.rng_words_match(f['rng'][0], st[slot]), f['name']
    return env


def step_build(env):
    """cc4_debug_step_build: (one-wave step kernel?, the four-wave step kernel's register budget, the multi-step build)."""
    out = (ctypes.c_int32 * 3)()
    env._chk(env.lib.cc4_debug_step_build(env._h, out), 'cc4_debug_step_build')
    return tuple(out)


def compare_slots(env, mode, placed, t, actions, what):
    """After t steps: every placed fixture's slot against the reference's arrays (observation row, reward, done, a zero error word, the last step's
    actions, the numpy stream's position) and against the oracle's hot row.  `actions`: [N, 5] the indices the last step ran with."""
    ora = oracle_replay(mode)
    env.synchronize()
    env._fetch()
    st = env.rng_state() if mode == 0 else None
    for f, slot in placed:
        tag = (what, f['name'], f'slot {slot}', f'after step {t - 1}')
        bad = np.nonzero(env._obs[slot] != f['obs'][t])[0]
        assert bad.size == 0, tag + ('observation values', bad[:12].tolist())
        assert env._rew[slot] == f['reward'][t - 1], tag + ('reward', float(env._rew[slot]), float(f['reward'][t - 1]))
        assert bool(env._done[slot]) == bool(f['done'][t - 1]), tag + ('done',)
        assert env._err[slot] == 0, tag + ('error word', hex(int(env._err[slot])))
        assert np.array_equal(actions[slot], f['actions'][t - 1]), tag + ('actions', actions[slot].tolist(), f['actions'][t - 1].tolist())
        if st is not None:
            assert G.rng_words_match(f['rng'][t], st[slot]), tag + ('PCG64 stream position',)
        row, want = env.get_state(slot), ora[f['name']]['hot'][t]
        if mode == 0:       # the numpy-stream handle holds its classes per episode (start_device): the row's assignment byte says so; the oracle had them as its argument
            want = want.copy()
            assert row_set(want, f['red_policy'], f['green_policy'], f['blue_policy']) == 0
        bad = np.nonzero(row != want)[0]
        assert bad.size == 0, tag + ('hot row bytes against the oracle', bad[:12].tolist())


def run_case(mode, n, which, kernel_for, stepper='random', groups=None, **kw):
    """One placement of one case.  kernel_for(k): the kernel a call of k steps must take on this handle (cc4_run_kernel_for; for the per-step ways of
    stepping, cc4_step_kernel).  stepper: 'random' cc4_run_random_steps; 'policy' the draw kernel plus cc4_step_device per step (run_policy_steps);
    'rollout' run_rollout(k, 'random', seed0, t) for the calls of ten steps and more ('k_run_philox1r'), cc4_run_random_steps for the shorter ones.
    Returns (env at its end, placed, {k: the kernel that served the call})."""
    seed0, placed = placement(mode, n, which)
    env = start_device(mode, n, placed, **kw)
    served, t = {}, 0
    try:
        for k in CALLS:
            want = kernel_for(k)
            if stepper == 'policy':
                assert env.step_kernel == want, (k, env.step_kernel)
                env.run_policy_steps(seed0, t, k)
                served[k] = env.step_kernel
            elif stepper == 'rollout' and k >= 10:
                assert env.run_kernel_for(k) == 'k_run_philox1', (k, env.run_kernel_for(k))       # the handle has the persistent schedule a rollout needs
                env.run_rollout(k, 'random', seed0, t)
                G_, blk = ctypes.c_int32(), ctypes.c_int32()
                assert env.lib.cc4_rollout_groups(env._h, ctypes.byref(G_), ctypes.byref(blk)) == 0 and G_.value == groups, G_.value
                served[k] = 'k_run_philox1r'       # (what persist_launch sends a rollout: cc4_rollout_begin has no other form)
            else:
                assert env.run_kernel_for(k) == want, (k, env.run_kernel_for(k), want)
                env.run_random_steps(seed0, t, k, timed=False)
                served[k] = want
            t += k
            actions = env.rollout_actions(k - 1) if served[k] == 'k_run_philox1r' else env.device_actions()
            compare_slots(env, mode, placed, t, actions, f'{which} placement, call of {k} steps ({served[k]})')
        assert t == STEPS
    except BaseException:
        env.close()
        raise
    return env, placed, served
