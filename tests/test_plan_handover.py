"""GPU: the hand-over between the waves of the persistent plan kernels, arbitrated by the CPU oracle.

The self-check (CC4_PERSIST_VERIFY) compares a persistent launch with per-step launches of a shadow handle and cannot say which side left the true
trajectory, nor where.  Here every cell of tests/handover_util.py -- `base`, the one call that has been seen disagreeing, and twelve cells that differ from
it in a single factor -- runs R times on one handle at the persistent kernels' own batch sizes, with no shadow beside it, and everything it produces is
compared exactly with the ONE trajectory the oracle computed for the cell: the recorded observations, rewards and dones of every step and episode, the error
words, every hot row, the generator states, a stride of cold rows.  The first mismatch fails the test with its place in the schedule -- (episode, step, run,
position q in the run, run length, regeneration?, partition) --, the repetition, and how many episodes differ at that step.  (Two cells record less:
`no_record` has no observation rows, and `random_steps` -- cc4_run_random_steps returns no trajectory -- is compared in the outputs of its last step, the
last actions drawn and the rows at its end only, so a mismatch there names episodes and partitions but no step.)

What does not depend on timing is asserted too: the kernel each call takes, the cell's premise (tests/test_plan_handover_cpu.py asserts the same at 8
episodes), clean error words.  The recorded observations stay packed (148 bytes a row) on both sides: the oracle's rows are packed once."""
import time

import numpy as np
import pytest

import handover_util as H

pytestmark = pytest.mark.gpu


def run_cell(cell, traj, reps):
    """The cell `reps` times on one fresh handle (its environment is the caller's business); None, or the first repetition's mismatch as text."""
    from cage_challenge_4_amd import CC4VecEnv
    n = cell.n
    env = CC4VecEnv(n, steps=cell.steps, rng_mode=cell.rng_mode, autoreset=True, strict=False)
    try:
        plan_kernel = 'k_run_pcgp' if cell.rng_mode == 0 else 'k_run_philox1p'
        for rep in range(reps):
            env.reset(seeds=H.RESET_SEED)
            for c, act, msg in traj.inputs[:-1]:
                assert env.plan_kernel_for(c.k) == plan_kernel, (cell.id, c)
                info = env.run_plan(act, msg, record_obs=c.record)[3]
                assert not info['err'].any(), (cell.id, rep, c)
            c, act, msg = traj.inputs[-1]
            seq = rew = done = None
            if isinstance(c, H.Plan):
                assert env.plan_kernel_for(c.k) == H.kernel_name(cell), cell.id
                obs, rew, done, info = env.run_plan(act, msg, record_obs=c.record)
                seq, err = info.get('obs_seq'), info['err'].copy()           # (packed rows: the caller replaced the module's unpacking)
                assert (seq is not None) == c.record
            else:
                assert env.run_kernel_for(c.k) == H.kernel_name(cell), cell.id
                env.run_random_steps(H.RANDOM_SEED0, H.RANDOM_T0, c.k, timed=False)
                obs = env._fetch()[0]
                err = env.err.copy()
                assert np.array_equal(env.device_actions(), act[-1]), (cell.id, rep)
            final = {'error words': (err, traj.err if isinstance(c, H.Plan) else traj.err_last), 'last observations': (obs, traj.obs_last), 'last rewards': (env._rew, traj.reward_last),
                     'last dones': (env._done.astype(bool), traj.done_last), 'hot rows': (env.get_states(), traj.hot), 'generator state': (env.rng_state(), traj.rng),
                     'cold rows': (np.stack([env.get_cold(e) for e in traj.cold]), np.stack(list(traj.cold.values())), list(traj.cold))}
            bad = H.first_mismatch(cell, traj, seq, rew, done, final)
            if bad:
                return f'{cell.id}, repetition {rep} of {reps}: {bad}'
            assert not err.any(), (cell.id, rep)
        return None
    finally:
        env.close()


@pytest.mark.parametrize('cid', list(H.CELLS))
def test_cell_matches_the_oracle_every_time(cid, monkeypatch):
    import cage_challenge_4_amd.vec_env as V
    cell = H.CELLS[cid]
    t0 = time.perf_counter()
    traj = H.oracle_trajectory(cell)
    H.check_premise(cell, traj)
    t1 = time.perf_counter()
    for k in ('CC4_PERSIST_VERIFY', 'CC4_PERSIST_THR', 'CC4_PERSIST_RUNS', 'CC4_PERSIST', 'CC4_PERSIST_MIN_K'):
        monkeypatch.delenv(k, raising=False)
    monkeypatch.setenv('CC4_PERSIST_VERIFY_EVERY', '0')          # no shadow handle beside the kernel
    for k, v in cell.knobs:                                       # (persist_setup reads them once, with the handle's first persistent call)
        monkeypatch.setenv(k, v)
    monkeypatch.setattr(V, 'unpack_obs_rows', lambda packed: packed)      # run_plan's info['obs_seq'] stays packed
    bad = run_cell(cell, traj, cell.R)
    t2 = time.perf_counter()
    print(f'\n[handover] {cid}: oracle {t1 - t0:.2f} s, {cell.R} repetitions {t2 - t1:.2f} s ({(t2 - t1) / cell.R:.3f} s each), {"DISAGREES: " + bad if bad else "agrees"}')
    assert bad is None, bad
