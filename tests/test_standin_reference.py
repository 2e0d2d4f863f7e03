"""GPU: the stand-in-action call path (cc4_run_random_steps: the blue actions drawn inside the kernel) against the REFERENCE, on every step build.

tests/golden/ctrstand_*.npz and trajstand_*.npz are reference episodes whose blue actions are the stand-in's own draws (golden_util.load_standin,
oracle/refgen/make_ctr_golden.py / make_golden.py `standin`).  Each case places them in the slots their action keys name (standin_util.placement), twice
-- 'low': the fixtures at their offsets, slot 0 included; 'high': the deepest fixture that fits in the batch's last slot -- steps the batch in calls of
1, 3, 9, 10, 12, 20 and 45 steps, and after every call compares each fixture's slot with the recorded observation row, reward, done, a zero error word,
the actions of the call's last step, and the hot row of an oracle handle that replayed the same fixture (a run call returns only its last step; the
row stands for the steps in between).  Every comparison is exact.  Every call names the kernel that serves it, every case the build it reached.

Not reached: k_run_philox1g -- persist_launch sends it only a persistent call that is not of the headline shape, and without a communicator every
cc4_run_random_steps call that takes the persistent form is of that shape (profile counters, the event log and submitted red / green actions all take
the per-step launches instead); k_run_philox1x needs a communicator."""
import numpy as np
import pytest

import standin_util as S

pytestmark = pytest.mark.gpu

BOTH = ('low', 'high')


def _setenv(monkeypatch, env):
    for k in ('CC4_PHILOX_LEAN', 'CC4_PHILOX_MINW', 'CC4_MULTISTEP', 'CC4_RUN1', 'CC4_GROUPS', 'CC4_PERSIST', 'CC4_PERSIST_MIN_K', 'CC4_PERSIST_VERIFY',
              'CC4_PERSIST_VERIFY_EVERY', 'CC4_ROLLOUT_GROUPS'):
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)


def _check_case(mode, n, count, target, kernel_for, build=None, **kw):
    """Both placements of a case: `count` fixtures placed in each, the first and the last slot of the batch each held one in one of them, `target` served
    the calls of 10, 12, 20 and 45 steps, and (build) cc4_debug_step_build's words: {index: value}."""
    slots = set()
    for which in BOTH:
        env, placed, served = S.run_case(mode, n, which, kernel_for, **kw)
        try:
            assert len(placed) == count, (which, [(f['name'], s) for f, s in placed])
            assert all(served[k] == target for k in S.LONG), served
            if build:
                got = S.step_build(env)
                assert all(got[i] == v for i, v in build.items()), (got, build)
            print(f'{target} {which}: {n} episodes, fixtures in slots {[s for _, s in placed]}, calls served by {served}, step build {S.step_build(env)}')
        finally:
            env.close()
        slots |= {s for _, s in placed}
    assert 0 in slots and n - 1 in slots, sorted(slots)


# ---------------------------------------------------------------------------------------------------------------- 96 episodes: the kernels of small batches
SMALL = [  # id, environment, the kernel of a call of one step, ... of two steps and more, cc4_debug_step_build words {index: value}
    ('k_run_philox', {'CC4_PHILOX_LEAN': '0'}, 'k_step_philox', 'k_run_philox', {0: 0, 1: 1, 2: 5}),
    ('k_run_philox8', {'CC4_PHILOX_LEAN': '0', 'CC4_MULTISTEP': '8'}, 'k_step_philox', 'k_run_philox8', {0: 0, 1: 1, 2: 8}),
    ('k_run_philox1m', {'CC4_PHILOX_LEAN': '1'}, 'k_step_philox1', 'k_run_philox1m', {0: 1}),
    ('k_step_philox-minw1', {'CC4_MULTISTEP': '0', 'CC4_RUN1': '0', 'CC4_PHILOX_MINW': '1'}, 'k_step_philox', 'k_step_philox', {0: 0, 1: 1}),
    ('k_step_philox-minw7', {'CC4_MULTISTEP': '0', 'CC4_RUN1': '0', 'CC4_PHILOX_MINW': '7'}, 'k_step_philox', 'k_step_philox', {0: 0, 1: 7}),
    ('k_step_philox-minw8', {'CC4_MULTISTEP': '0', 'CC4_RUN1': '0', 'CC4_PHILOX_MINW': '8'}, 'k_step_philox', 'k_step_philox', {0: 0, 1: 8}),
    ('k_step_philox1', {'CC4_PHILOX_LEAN': '1', 'CC4_MULTISTEP': '0', 'CC4_RUN1': '0'}, 'k_step_philox1', 'k_step_philox1', {0: 1}),
]


@pytest.mark.parametrize('case', SMALL, ids=[c[0] for c in SMALL])
def test_small_batch_kernels_replay_the_reference(case, monkeypatch):
    """96 episodes, counter mode: the multi-step kernels (k_run_philox, k_run_philox8, k_run_philox1m) and the fused draw of the per-step launches
    (k_step_philox at the register budgets 1, 7 and 8; k_step_philox1).  Six fixtures in each placement (offsets 0 .. 64)."""
    _, env, one, more, build = case
    _setenv(monkeypatch, env)
    _check_case(1, 96, 6, more, lambda k: one if k < 2 else more, build=build)


@pytest.mark.parametrize('case', SMALL[3:], ids=[c[0] for c in SMALL[3:]])
def test_draw_kernel_and_device_step_replay_the_reference(case, monkeypatch):
    """The same per-step builds stepped as a learner's loop does: k_random_actions writes the draws, cc4_step_device consumes them (run_policy_steps)."""
    _, env, one, more, build = case
    _setenv(monkeypatch, env)
    _check_case(1, 96, 6, more, lambda k: more, build=build, stepper='policy')


def test_numpy_stream_step_kernel_replays_the_reference(monkeypatch):
    """96 episodes on the numpy stream (k_step, per-step launches): the fixtures of offsets 0 and 64, the PCG64 stream position included."""
    _setenv(monkeypatch, {})
    _check_case(0, 96, 2, 'k_step', lambda k: 'k_step')


# ---------------------------------------------------------------------------------------------------------------- 6656 episodes: the persistent kernels
N_PERSIST = 6656          # the smallest batch the persistent kernels take in this suite


def test_headline_kernel_replays_the_reference(monkeypatch):
    """k_run_philox1, the build bench.py times: calls of ten steps and more run it, shorter ones the per-step kernel.  The sampled self-check stays at
    its default.  All nine fixtures in both placements."""
    _setenv(monkeypatch, {})
    _check_case(1, N_PERSIST, 9, 'k_run_philox1', lambda k: 'k_run_philox1' if k >= 10 else 'k_step_philox1', build={0: 1})


def test_numpy_stream_persistent_kernel_replays_the_reference(monkeypatch):
    """k_run_pcg with the trajstand_* episodes, the PCG64 stream position after every call included."""
    _setenv(monkeypatch, {})
    _check_case(0, N_PERSIST, 3, 'k_run_pcg', lambda k: 'k_run_pcg' if k >= 10 else 'k_step')


@pytest.mark.parametrize('groups', [1, 4])
def test_rollout_kernel_replays_the_reference(groups, monkeypatch):
    """k_run_philox1r: the calls of ten steps and more are rollouts with the stand-in policy in the loop (the policy kernel's draws, published per policy
    group), the shorter ones cc4_run_random_steps.  The actions compared are those of the rollout's last action slot."""
    _setenv(monkeypatch, {'CC4_ROLLOUT_GROUPS': str(groups)})
    _check_case(1, N_PERSIST, 9, 'k_run_philox1r', lambda k: 'k_step_philox1', stepper='rollout', groups=groups)
