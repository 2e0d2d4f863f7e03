"""GPU: the wave-wide phases of the numpy-stream kernels (cc4_k_pcg.hip: wave_green_policy, wave_shuffle_consume, wave_green_exec) at crafted
generator states (tests/pcg_craft.py).  Those phases compute from the LCG's closed form what the engine's serial walk draws one by one, and hand
to the walking lane what the speculation cannot settle: a zero word in a bounded draw (Lemire's re-draw, n / 2^32 per draw), a zero buffered half
word, a 1 % event that needs a port.  Seeds meet these about never; a planted output meets them at a known offset.  Every episode gets one planted
output (five kinds x offsets 1..192 x four entry buffers) on both sides through set_generators; the reference is the oracle's serial walk, which
test_pcg_rare_draws_cpu.py ties to numpy at these very states.  Every comparison is exact."""
import numpy as np
import pytest

import pcg_craft as C
from cage_challenge_4_amd.vec_env import pcg64_words
from oracle_binding import OracleVecEnv, random_actions
from plan_util import random_plan

pytestmark = pytest.mark.gpu


def _pair(n, steps=C.STEPS, **kw):
    from cage_challenge_4_amd import CC4VecEnv
    return CC4VecEnv(n, steps=steps, rng_mode=0, strict=False, **kw), OracleVecEnv(n, steps=steps, rng_mode=0, **kw)


def _cell(cells, e):
    k, d, b = cells[e]
    return int(e), C.KINDS[k], int(d), C.BUFFERS[b]


def _differing(x, y, cells):
    """None, or the first episodes whose rows differ as (episode, planted kind, offset, entry buffer)."""
    n = len(cells)
    bad = np.nonzero((np.asarray(x).reshape(n, -1) != np.asarray(y).reshape(n, -1)).any(axis=1))[0]
    return None if bad.size == 0 else (int(bad.size), [_cell(cells, e) for e in bad[:6]])


def _assert_same(dev, ora, out_dev, out_ora, cells, where):
    """Observations, rewards, dones, error words, all seven generator words and every hot row."""
    for what, x, y in (('observations', out_dev[0], out_ora[0]), ('rewards', out_dev[1], out_ora[1]), ('dones', out_dev[2], out_ora[2]),
                       ('error words', out_dev[3], out_ora[3])):
        assert _differing(x, y, cells) is None, (where, what, _differing(x, y, cells))
    assert not np.asarray(out_ora[3]).any(), (where, 'the oracle raised an error word')
    assert _differing(dev.rng_state(), ora.rng_state(), cells) is None, (where, 'generator words', _differing(dev.rng_state(), ora.rng_state(), cells))
    rows, want = dev.get_states(), np.stack([ora.get_state(i) for i in range(len(cells))])
    assert _differing(rows, want, cells) is None, (where, 'hot rows', _differing(rows, want, cells))


def _warm_up_and_plant(dev, ora, n, seed, actions=lambda t, n: random_actions(C.ACT_SEED, t, n), evlog=False):
    """Same seeds, 25 steps with the same actions (red agents hold sessions, greens have services to pick from), then one crafted generator per
    episode on the increment its stream already has, the same objects to both sides.  Returns the cells [n, 3] (kind, offset, buffer)."""
    assert np.array_equal(dev.reset(seeds=C.SEED0), ora.reset_batch(C.SEED0))
    if evlog:
        dev.enable_event_log(), ora.enable_event_log()
    for t in range(C.WARMUP):
        a = actions(t, n)
        d, o = dev.step(a), ora.step_batch(a)
    assert np.array_equal(d[0], o[0]) and np.array_equal(dev.rng_state(), ora.rng_state()), 'the handles differ before anything is planted'
    cells = C.batch_cells(n)
    gens = C.crafted_generators(ora.rng_state(), cells, seed=seed)
    dev.set_generators(gens), ora.set_generators(gens)
    want = np.array([pcg64_words(g) + [0] for g in gens], dtype=np.uint64)      # (the advance count restarts where the state is set)
    assert np.array_equal(dev.rng_state(), want) and np.array_equal(ora.rng_state(), want)
    return cells


def _flat(out):
    return out[0], out[1], out[2], out[3]['err']


# ---------------------------------------------------------------------------------------------------------------- per-step launches
@pytest.mark.parametrize('name', list(C.CASES))
def test_step_kernel_at_planted_states(name):
    """k_step<false> with the caller's blue actions and with the built-in random blue (its draws come first and shift every phase); k_step<true>
    (event log on: wave_green_policy and wave_shuffle_consume stay wave-wide, the green actions walk on lane 0); SleepAgent greens (the walk
    behind `!drawn` is the ordinary path there).  Compared after every step."""
    case = C.CASES[name]
    n = case['n']
    dev, ora = _pair(n, **case['kw'])
    assert dev.step_kernel == 'k_step'
    cells = _warm_up_and_plant(dev, ora, n, case['seed'], actions=lambda t, n: C.case_actions(case, t, n), evlog=case['evlog'])
    for t in range(C.WARMUP, C.WARMUP + case['steps']):
        a = C.case_actions(case, t, n)
        _assert_same(dev, ora, _flat(dev.step(a)), _flat(ora.step_batch(a)), cells, (name, 'step', t - C.WARMUP + 1))
    # every episode met its planted output (test_pcg_rare_draws_cpu.py asserts the same of the oracle alone)
    adv = ora.rng_state()[:, 6].astype(np.int64)
    assert (adv >= cells[:, 1]).all(), [_cell(cells, e) for e in np.nonzero(adv < cells[:, 1])[0][:6]]
    dev.close(), ora.close()


# ---------------------------------------------------------------------------------------------------------------- one launch for the whole call
# the batch the suite already runs the persistent numpy-stream kernels at; 100-step episodes (the cold rows of 8192 500-step episodes take the oracle
# seconds to allocate): the second mission phase begins at step 33, between the planted steps
N_PERSIST, K_PERSIST, STEPS_PERSIST = 8192, 12, 100


def test_persistent_kernel_at_planted_states():
    """k_run_pcg: one cc4_run_random_steps call of 12 steps against 12 oracle steps with the actions the call draws."""
    n, k, seed0 = N_PERSIST, K_PERSIST, 31
    dev, ora = _pair(n, steps=STEPS_PERSIST)
    assert dev.run_kernel_for(k) == 'k_run_pcg'
    cells = _warm_up_and_plant(dev, ora, n, seed=5)
    dev.run_random_steps(seed0, C.WARMUP, k, timed=False)
    for j in range(k):
        a = random_actions(seed0, C.WARMUP + j, n)
        o = ora.step_batch(a)
    dev.synchronize(), dev._fetch()
    assert np.array_equal(dev.device_actions(), a), 'the actions the call reports for its last step'
    _assert_same(dev, ora, (dev._obs, dev._rew, dev._done.astype(bool), dev._err), _flat(o), cells, 'k_run_pcg')
    dev.close(), ora.close()


def test_persistent_plan_kernel_at_planted_states():
    """k_run_pcgp: one run_plan of 12 random rows; the per-step rewards and dones it returns, and the handle at the end."""
    n, k = N_PERSIST, K_PERSIST
    dev, ora = _pair(n, steps=STEPS_PERSIST)
    assert dev.plan_kernel_for(k) == 'k_run_pcgp'
    cells = _warm_up_and_plant(dev, ora, n, seed=6)
    plan = random_plan(np.random.default_rng(12), k, n)[0]
    obs, rew, done, info = dev.run_plan(plan)
    for j in range(k):
        o = ora.step_batch(plan[j])
        assert _differing(rew[j], o[1], cells) is None, ('rewards of plan step', j, _differing(rew[j], o[1], cells))
        assert _differing(done[j], o[2], cells) is None, ('dones of plan step', j, _differing(done[j], o[2], cells))
    _assert_same(dev, ora, (obs, rew[-1], done[-1], info['err']), _flat(o), cells, 'k_run_pcgp')
    dev.close(), ora.close()
