"""GPU: the hand-over between the waves of the persistent plan kernels, arbitrated by the CPU oracle.

The self-check (CC4_PERSIST_VERIFY) compares a persistent launch with per-step launches of a shadow handle and cannot say which side left the true
trajectory, nor where.  Here every cell of tests/handover_util.py -- `base`, the one call that has been seen disagreeing, and twelve cells that differ from
it in a single factor -- runs R times on one handle at the persistent kernels' own batch sizes, with nothing beside it, and everything it produces is
compared exactly with the ONE trajectory the oracle computed for the cell: the recorded observations, rewards and dones of every step and episode, the error
words, every hot row, the generator states, a stride of cold rows.  The first mismatch fails the test with its place in the schedule -- (episode, step, run,
position q in the run, run length, regeneration?, partition) --, the repetition, and how many episodes differ at that step.  (Two cells record less:
`no_record` has no observation rows, and `random_steps` -- cc4_run_random_steps returns no trajectory -- is compared in the outputs of its last step, the
last actions drawn and the rows at its end only, so a mismatch there names episodes and partitions but no step.)

Six further cells reuse those inputs and trajectories with SOMETHING BESIDE THE KERNEL (Cell.beside), the one thing the failing call had that the cells
above lack.  `selfcheck_all` / `selfcheck_last` / `selfcheck_pcg` / `selfcheck_random` create the handle with the self-check on, so that the shadow handle's
per-step launches are enqueued beside the persistent kernel exactly as in the failing test; the calls go through handover_util's raw driver, which keeps
what a disagreeing call produced, and the oracle arbitrates: a repetition passes only if the call returned 0 and the main side equals the trajectory, and a
-5 is reported as SHADOW LEFT THE TRAJECTORY or KERNEL LEFT THE TRAJECTORY with the episodes, the partitions and the self-check's own message in full.
`neighbour_after` / `neighbour_before` put a second handle's per-step plan call on the device right behind / in front of the kernel, compare both handles with
the trajectory, and print (never assert) the share of the kernel's call during which the neighbour's launches were in flight.

What does not depend on timing is asserted too: the kernel each call takes, the cell's premise (tests/test_plan_handover_cpu.py asserts the same at 8
episodes), clean error words.  The recorded observations stay packed (148 bytes a row) on both sides: the oracle's rows are packed once."""
import ctypes
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


def _last_error(env):
    msg = env.lib.cc4_last_error(env._h)
    return msg.decode() if msg else ''


def _prefix_calls(cell, traj, env, rep, reps, kernel):
    """The plan calls in front of the call under test, through the raw driver (a checked one that disagrees returns -5 instead of raising); None, or why
    the repetition ends here.  The oracle keeps no trajectory of these calls, so a disagreement in one of them is quoted, not arbitrated."""
    for c, act, msg in traj.inputs[:-1]:
        assert env.plan_kernel_for(c.k) == kernel, (cell.id, c, kernel)
        res = H.run_plan_raw(env, act, msg, record_obs=c.record)
        if res.rc:
            return f'{cell.id}, repetition {rep} of {reps}: the {c.k}-step plan call in front of the call under test returned {res.rc}: "{res.error}"'
        err = np.zeros(cell.n, np.uint32)
        env._chk(env.lib.cc4_get_err(env._h, err.ctypes.data_as(ctypes.c_void_p)), 'cc4_get_err')
        assert not err.any(), (cell.id, rep, c)
    return None


def run_selfcheck_cell(cell, traj, reps):
    """A cell whose handle was created with a self-check setting (the caller's environment), `reps` times: every checked call runs the shadow handle's
    per-step launches beside the kernel.  (None or the first repetition's verdict as text, (calls checked, calls that disagreed)).  A repetition passes only
    if the call returned 0 AND the main handle's side equals the oracle (H.self_check_verdict names the side otherwise)."""
    from cage_challenge_4_amd import CC4VecEnv
    env = CC4VecEnv(cell.n, steps=cell.steps, rng_mode=cell.rng_mode, autoreset=True, strict=False)
    try:
        plan = isinstance(cell.call, H.Plan)
        c, act, msg = traj.inputs[-1]
        bad = None
        for rep in range(reps):
            env.reset(seeds=H.RESET_SEED)
            bad = _prefix_calls(cell, traj, env, rep, reps, 'k_run_pcgp' if cell.rng_mode == 0 else 'k_run_philox1p')
            if bad:
                break
            if plan:
                assert env.plan_kernel_for(c.k) == H.kernel_name(cell), cell.id
                res = H.run_plan_raw(env, act, msg, record_obs=c.record)
                rc, error = res.rc, res.error
                main = H.Side(res.obs_packed, res.rewards, res.dones, H.fetch_final(env.lib, env._h, traj, True))
            else:
                assert env.run_kernel_for(c.k) == H.kernel_name(cell), cell.id
                rc = int(env.lib.cc4_run_random_steps(env._h, ctypes.c_uint64(H.RANDOM_SEED0), ctypes.c_uint32(H.RANDOM_T0), c.k, None))
                error = _last_error(env) if rc else None
                final = H.fetch_final(env.lib, env._h, traj, False)
                final['last actions drawn'] = (env.device_actions(), np.asarray(act[-1], np.int32))
                main = H.Side(final=final)
            sh = H.shadow_handle(env)
            assert sh is not None, (cell.id, 'the handle has no shadow: nothing ran beside the kernel')
            bad = H.self_check_verdict(cell, traj, rc, error, main)
            if bad:                      # (the shadow's side is fetched only where there is something to say about it)
                bad = H.self_check_verdict(cell, traj, rc, error, main, H.Side(final=H.fetch_final(env.lib, sh, traj, plan)))
                bad = f'{cell.id}, repetition {rep} of {reps}: {bad}'
                break
            assert not main.final['error words'][0].any(), (cell.id, rep)
        return bad, env.verify_stats()
    finally:
        env.close()


def run_neighbour_cell(cell, traj, reps, monkeypatch):
    """Handle A makes the cell's call (the persistent kernel, no self-check); handle B -- the same configuration, reset seed and calls in front, created
    with CC4_PERSIST=0 -- takes the same plan in the per-step form, enqueued right behind A's call (`after`) or right in front of it (`before`) with no
    host wait in between; both are synchronised afterwards and each is compared with the cell's trajectory.  (None or the first repetition's verdict,
    [(share of A's call during which B's launches were in flight, ms A's call took on its stream, ms B's launches took on theirs), per repetition]) -- measured
    with events on the two main streams, reported, never asserted: whether two handles' streams overlap is the machine's business."""
    from cage_challenge_4_amd import CC4VecEnv
    kw = dict(steps=cell.steps, rng_mode=cell.rng_mode, autoreset=True, strict=False)
    A = CC4VecEnv(cell.n, **kw)
    B = None
    try:
        monkeypatch.setenv('CC4_PERSIST', '0')
        try:
            B = CC4VecEnv(cell.n, **kw)
        finally:
            monkeypatch.delenv('CC4_PERSIST')
        c, act, msg = traj.inputs[-1]
        shares, bad = [], None
        for rep in range(reps):
            for env, kernel in ((A, 'k_run_pcgp' if cell.rng_mode == 0 else 'k_run_philox1p'), (B, B.step_kernel)):
                env.reset(seeds=H.RESET_SEED)
                bad = bad or _prefix_calls(cell, traj, env, rep, reps, kernel)
            if bad:
                break
            assert A.plan_kernel_for(c.k) == H.kernel_name(cell) and B.plan_kernel_for(c.k) == B.step_kernel, cell.id
            calls = {'a': (A, H.PlanCall(A, act, msg, c.record)), 'b': (B, H.PlanCall(B, act, msg, c.record))}
            A.synchronize()
            B.synchronize()
            clock = H.StreamTimes(A)
            try:
                for tag in ('ab' if cell.beside.order == 'after' else 'ba'):
                    env, call = calls[tag]
                    clock.mark(tag + '0', env)
                    call.enqueue()
                    clock.mark(tag + '1', env)
            finally:
                got = {tag: call.finish() if call.rc is not None else call._free() for tag, (env, call) in calls.items()}
            t = clock.times()
            shares.append((H.overlap_share(t['a0'], t['a1'], t['b0'], t['b1']), t['a1'] - t['a0'], t['b1'] - t['b0']))
            sides = [(r.rc, r.error, H.Side(r.obs_packed, r.rewards, r.dones, H.fetch_final(env.lib, env._h, traj, True)) if r.rc == 0 else None)
                     for env, r in ((A, got['a']), (B, got['b']))]
            bad = H.neighbour_verdict(cell, traj, *sides)
            if bad:
                bad = f'{cell.id}, repetition {rep} of {reps}: {bad}'
                break
        return bad, shares
    finally:
        A.close()
        if B is not None:
            B.close()


def test_a_real_mismatch_message_is_arbitrated_like_the_canned_one(monkeypatch):
    """tests/test_plan_handover_cpu.py feeds self_check_verdict a canned message; here the library writes it.  `selfcheck_all` once, with one byte of the
    SHADOW's recorded packed row of step 69, episode 6 changed between the runs and the compare (cc4_debug_verify_plant, include/cc4_debug.h: data only,
    never stepped) -- the canned message's trajectory clause.  The call returns -5 with that clause, and the verdict, which sees both sides equal to the
    oracle in everything fetched, places the difference in the shadow's recorded rows."""
    cell = H.CELLS['selfcheck_all']
    traj = H.oracle_trajectory(cell)
    for k in ('CC4_PERSIST_VERIFY_EVERY', 'CC4_PERSIST_THR', 'CC4_PERSIST_RUNS', 'CC4_PERSIST', 'CC4_PERSIST_MIN_K'):
        monkeypatch.delenv(k, raising=False)
    monkeypatch.setenv(cell.beside.env, cell.beside.value)
    from cage_challenge_4_amd import CC4VecEnv
    env = CC4VecEnv(cell.n, steps=cell.steps, rng_mode=cell.rng_mode, autoreset=True, strict=False)
    try:
        env.reset(seeds=H.RESET_SEED)
        assert _prefix_calls(cell, traj, env, 0, 1, 'k_run_philox1p') is None
        c, act, msg = traj.inputs[-1]
        assert env.plan_kernel_for(c.k) == H.kernel_name(cell) and (c.k, c.record) == (70, True)
        assert env.lib.cc4_debug_verify_plant(env._h, 9, 6, 3, 69) == 0
        res = H.run_plan_raw(env, act, msg, record_obs=True)
        said = ('CC4_PERSIST_VERIFY: k_run_philox1p and the per-step launches disagree after a plan of 70 steps: first differing trajectory row: packed '
                'observations of step 69, 1 episode(s) differ in it, first episode 6')
        assert (res.rc, res.error) == (H.VERIFY_MISMATCH, said)
        main = H.Side(res.obs_packed, res.rewards, res.dones, H.fetch_final(env.lib, env._h, traj, True))
        shadow = H.Side(final=H.fetch_final(env.lib, H.shadow_handle(env), traj, True))
        verdict = H.self_check_verdict(cell, traj, res.rc, res.error, main, shadow)
        assert verdict.startswith('SHADOW LEFT THE TRAJECTORY') and 'KERNEL' not in verdict and f'"{said}"' in verdict, verdict
        assert 'the difference lies in its recorded trajectory rows alone' in verdict, verdict
        assert env.verify_stats() == (len(cell.prefix) + 1, 1)
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
    monkeypatch.setenv('CC4_PERSIST_VERIFY_EVERY', '0')          # no shadow handle beside the kernel ..
    if isinstance(cell.beside, H.SelfCheck):                     # .. unless that is the cell (read at cc4_create)
        monkeypatch.setenv(cell.beside.env, cell.beside.value)
    for k, v in cell.knobs:                                       # (persist_setup reads them once, with the handle's first persistent call)
        monkeypatch.setenv(k, v)
    monkeypatch.setattr(V, 'unpack_obs_rows', lambda packed: packed)      # run_plan's info['obs_seq'] stays packed
    beside = ''
    if isinstance(cell.beside, H.SelfCheck):
        bad, (checked, disagreed) = run_selfcheck_cell(cell, traj, cell.R)
        beside = f'{checked} call(s) checked with the shadow beside the kernel, {disagreed} disagreed, '
        if not bad:        # every call checked, or the call under test alone (a repetition is len(prefix) + 1 persistent calls)
            want = cell.R * (len(cell.prefix) + 1) if cell.beside.env == 'CC4_PERSIST_VERIFY' else cell.R
            assert (checked, disagreed) == (want, 0), (cid, checked, disagreed, want)
    elif isinstance(cell.beside, H.Neighbour):
        bad, shares = run_neighbour_cell(cell, traj, cell.R, monkeypatch)
        known = sorted(s for s, _, _ in shares if s is not None)
        mid = lambda v: sorted(v)[len(v) // 2]          # noqa: E731
        beside = (f'overlap share (of A\'s call, B\'s launches in flight) min {known[0]:.2f} / median {mid(known):.2f} / max {known[-1]:.2f} over {len(known)} repetition(s); '
                  f'on their streams A\'s call took {mid([a for _, a, _ in shares]):.2f} ms, B\'s launches {mid([b for _, _, b in shares]):.2f} ms (medians), '
                  if known else 'overlap share not measured, ')
    else:
        bad = run_cell(cell, traj, cell.R)
    t2 = time.perf_counter()
    print(f'\n[handover] {cid}: oracle {t1 - t0:.2f} s, {cell.R} repetitions {t2 - t1:.2f} s ({(t2 - t1) / cell.R:.3f} s each), {beside}{"DISAGREES: " + bad if bad else "agrees"}')
    assert bad is None, bad
