"""The host API's entry prologue, its group fork and what a handle owns, from outside the library.

Refusals: with a rollout in flight every entry point either refuses -- -2 with its own name in cc4_last_error, or -1 from the join every call goes
through, whose sentence names nobody -- or, for the few that touch neither the rows nor the streams, passes.  The table below is what the library
did before the prologue was stated once (csrc/cc4_api.hip enter); it is kept as literals.  After cc4_rollout_end the same calls succeed.
(cc4_rollout_begin needs the persistent kernel, which a batch the chip holds at once never takes: the handle is the 6656 episodes tests/test_plan.py
begins its rollout on, not 64.  The "not on a handle with a communicator" refusals are checked on a second, four-episode handle with a one-rank
communicator, as tests/test_plan.py and tests/test_episode_copy.py make theirs.)

Group fork: three group streams on 64 episodes (CC4_GROUPS=3), one handle through every call that orders the group streams behind the main one
(cc4_step_device, cc4_step_group_device, cc4_run_random_steps with the enqueue threads and without, timed and untimed) with main-stream work in
between, against the oracle after every call.

Resources: what the handles of this process own returns to where it stood once they are destroyed (cc4_debug_live_resources)."""
import ctypes
import os

import numpy as np
import pytest
from oracle_binding import random_actions
from test_call_sequences import Pair, _fail

pytestmark = pytest.mark.gpu
VP = ctypes.c_void_p


class Scratch:
    """One device allocation of the test's own, carved into 256-byte aligned pieces."""

    def __init__(self, nbytes, device=0):
        from cage_challenge_4_amd.vec_env import _hip, _hip_chk
        self.hip, self.base, self.used, self.size = _hip(), VP(), 0, nbytes
        _hip_chk(self.hip.hipSetDevice(device), 'hipSetDevice')
        _hip_chk(self.hip.hipMalloc(ctypes.byref(self.base), nbytes), 'hipMalloc')

    def take(self, nbytes):
        p = VP(self.base.value + self.used)
        self.used += (nbytes + 255) // 256 * 256
        assert self.used <= self.size
        return p

    def upload(self, arr):
        p = self.take(arr.nbytes)
        assert self.hip.hipMemcpy(p, arr.ctypes.data_as(VP), arr.nbytes, 1) == 0
        return p

    def free(self):
        self.hip.hipFree(self.base)


def _calls(env, sc):
    """[(name, call, rc with a rollout in flight, cc4_last_error names the entry point, rc behind cc4_rollout_end)]; None: not called then."""
    lib, h, n = env.lib, env._h, env.num_envs
    sb, cb = int(lib.cc4_state_bytes()), int(lib.cc4_cold_bytes(h))
    host = {k: np.zeros(s, t) for k, s, t in (('obs', (n, 578), np.int32), ('rew', n, np.float32), ('done', n, np.uint8), ('err', n, np.uint32),
                                              ('mask', (n, 570), np.uint8), ('rng', (n, 7), np.uint64), ('act', (n, 5), np.int32),
                                              ('pol', (2, n, 3), np.int8), ('hot', sb, np.uint8), ('cold', cb, np.uint8), ('topo', 27 + 2 * 137, np.uint8),
                                              ('dig', (n, 3), np.uint64), ('word', 4, np.uint32))}
    hp = {k: v.ctypes.data_as(VP) for k, v in host.items()}
    seeds = np.arange(1, n + 1, dtype=np.uint64)
    idx = np.array([1, 2], np.int32)           # clone episode 1 into episode 2
    keep = np.full(n, -1, np.int8)             # CC4_POLICY_KEEP: an assignment that changes nothing
    d_act = VP()
    assert lib.cc4_actions_device(h, ctypes.byref(d_act)) == 0
    d_keep, d_pol = sc.upload(keep), sc.take(6 * n)
    d_idx = sc.upload(idx)
    d_out, d_out2 = sc.take(1 << 16), sc.take(1 << 16)
    d_po = [sc.take(b) for b in (n * 578, n * 570, n * 4, n, n * 4)]
    d_red = sc.upload(np.full((n, 6, 4), -1, np.int32))
    d_plan = sc.upload(np.zeros((1, n, 5), np.int32))
    d_seeds = sc.upload(seeds)
    json = ctypes.create_string_buffer(1 << 20)
    ident = (ctypes.c_uint8 * 128)()
    s0, u0 = ctypes.c_uint64(5), ctypes.c_uint32(0)

    def got_state():          # (cc4_set_state / cc4_set_cold below write back what these read: behind the rollout, rows the handle holds)
        return lib.cc4_get_state(h, 0, hp['hot']) or lib.cc4_get_cold(h, 0, hp['cold'])

    view = lambda f: (lambda: f(h, None, 0, None, 1, d_out, d_out2))       # noqa: E731
    return [
        ('cc4_reset', lambda: lib.cc4_reset(h, None, None), -1, False, 0),
        ('cc4_reset_device', lambda: lib.cc4_reset_device(h, d_seeds, None), -2, True, 0),
        ('cc4_set_policies_device', lambda: lib.cc4_set_policies_device(h, d_keep, None, None), -2, True, 0),
        ('cc4_set_policies', lambda: lib.cc4_set_policies(h, keep.ctypes.data_as(VP), None, None), -2, True, 0),
        ('cc4_policies_device', lambda: lib.cc4_policies_device(h, d_pol, None), -2, True, 0),
        ('cc4_get_policies', lambda: lib.cc4_get_policies(h, hp['pol'], None), -2, True, 0),
        ('cc4_step', lambda: lib.cc4_step(h, hp['act'], None), -1, False, 0),
        ('cc4_fetch', lambda: lib.cc4_fetch(h, hp['obs'], hp['rew'], hp['done'], hp['err']), -1, False, 0),
        ('cc4_step_fetch', lambda: lib.cc4_step_fetch(h, hp['act'], None, hp['obs'], hp['rew'], hp['done'], hp['err']), -1, False, 0),
        ('cc4_step_ex', lambda: lib.cc4_step_ex(h, hp['act'], None, None, None), -1, False, 0),
        ('cc4_edit_state', lambda: lib.cc4_edit_state(h, 0, 7, 3, 0, 0), -1, False, 0),
        ('cc4_get_obs', lambda: lib.cc4_get_obs(h, hp['obs']), -1, False, 0),
        ('cc4_get_reward_done', lambda: lib.cc4_get_reward_done(h, hp['rew'], hp['done']), -1, False, 0),
        ('cc4_get_action_mask', lambda: lib.cc4_get_action_mask(h, hp['mask']), -1, False, 0),
        ('cc4_get_err', lambda: lib.cc4_get_err(h, hp['err']), -1, False, 0),
        ('cc4_get_rng_state', lambda: lib.cc4_get_rng_state(h, hp['rng']), -1, False, 0),
        ('cc4_set_seed', lambda: lib.cc4_set_seed(h, seeds.ctypes.data_as(VP)), -1, False, 0),
        ('cc4_set_rng_state', lambda: lib.cc4_set_rng_state(h, hp['rng']), -2, True, -2),          # (a counter-mode handle: its own refusal comes first)
        ('cc4_get_actions', lambda: lib.cc4_get_actions(h, hp['act']), -1, False, 0),
        ('cc4_random_actions_device', lambda: lib.cc4_random_actions_device(h, s0, u0), -1, False, 0),
        ('cc4_stream_wait', lambda: lib.cc4_stream_wait(h, None), -1, True, 0),
        ('cc4_stream_signal', lambda: lib.cc4_stream_signal(h, None), -1, False, 0),
        ('cc4_policy_outputs', lambda: lib.cc4_policy_outputs(h, 0, *d_po), -1, False, 0),
        ('cc4_copy_episodes_device', lambda: lib.cc4_copy_episodes_device(h, 1, None, 0, d_idx, None, 0, VP(d_idx.value + 4), None), -2, True, 0),
        ('cc4_copy_faults', lambda: lib.cc4_copy_faults(h, hp['word']), -1, False, 0),
        ('cc4_clone_episodes', lambda: lib.cc4_clone_episodes(h, 1, idx.ctypes.data_as(VP), idx[1:].ctypes.data_as(VP), None), -2, True, 0),
        ('cc4_synchronize', lambda: lib.cc4_synchronize(h), -1, True, 0),
        ('cc4_get_state', lambda: lib.cc4_get_state(h, 0, hp['hot']), -1, False, 0),
        ('cc4_get_states', lambda: lib.cc4_get_states(h, 0, 1, hp['hot']), -1, False, 0),
        ('cc4_get_cold', lambda: lib.cc4_get_cold(h, 0, hp['cold']), -1, False, 0),
        ('cc4_set_state', lambda: got_state() or lib.cc4_set_state(h, 0, hp['hot']), -1, False, 0),
        ('cc4_set_cold', lambda: got_state() or lib.cc4_set_cold(h, 0, hp['cold']), -1, False, 0),
        ('cc4_get_topology', lambda: lib.cc4_get_topology(h, 0, hp['topo']), -1, False, 0),
        ('cc4_get_true_state', lambda: min(0, lib.cc4_get_true_state(h, 0, json, len(json))), -1, False, 0),
        ('cc4_enable_event_log', lambda: lib.cc4_enable_event_log(h, 0), -1, False, 0),
        ('cc4_keep_previous', lambda: lib.cc4_keep_previous(h, 0), 0, False, 0),                    # (switching it off touches nothing)
        ('cc4_replay_logged', lambda: lib.cc4_replay_logged(h), -2, True, -2),                       # (cc4_keep_previous is off: its own refusal)
        ('cc4_state_features_device', view(lib.cc4_state_features_device), -2, True, 0),
        ('cc4_red_view_device', view(lib.cc4_red_view_device), -2, True, 0),
        ('cc4_blue_view_device', view(lib.cc4_blue_view_device), -2, True, 0),
        ('cc4_blue_edges_device', lambda: lib.cc4_blue_edges_device(h, None, 0, None, 1, 160, d_out, d_out2), -2, True, 0),
        ('cc4_reward_terms_device', view(lib.cc4_reward_terms_device), -2, True, 0),
        ('cc4_sample_actions_device', lambda: lib.cc4_sample_actions_device(h, None, 0, None, 1, 3, None, s0, u0, 1.0, 2, d_out, d_out2), -2, True, 0),
        ('cc4_enable_reward_terms', lambda: lib.cc4_enable_reward_terms(h, 0), -2, True, 0),
        ('cc4_run_random_steps', lambda: lib.cc4_run_random_steps(h, s0, u0, 12, None), -1, False, 0),
        ('cc4_run_plan_device', lambda: lib.cc4_run_plan_device(h, 1, d_plan, None, None, None, None), -2, True, 0),
        ('cc4_unpack_rows_device', lambda: lib.cc4_unpack_rows_device(h, 1, d_out, 0, d_out2), -1, False, 0),
        ('cc4_rollout_begin', lambda: lib.cc4_rollout_begin(h, 1), -2, True, None),
        ('cc4_comm_init', lambda: lib.cc4_comm_init(h, 0, 1, ident), -1, False, None),
        ('cc4_allgather_obs', lambda: lib.cc4_allgather_obs(h, None), -2, True, -2),                # (no communicator: its own refusal)
        ('cc4_debug_profile', lambda: lib.cc4_debug_profile(h, 0, None), -1, False, 0),
        ('cc4_debug_stop_phase', lambda: lib.cc4_debug_stop_phase(h, 0), -1, False, 0),
        ('cc4_debug_persist_base', lambda: lib.cc4_debug_persist_base(h, 0), -2, True, 0),
        ('cc4_debug_copy_from_device', lambda: lib.cc4_debug_copy_from_device(h, hp['word'], d_out, 4), -1, False, 0),
        ('cc4_debug_digest', lambda: lib.cc4_debug_digest(h, hp['dig']), -1, False, 0),
        # (last: a handle that has taken red actions keeps the full builds of its kernels)
        ('cc4_step_red_device', lambda: lib.cc4_step_red_device(h, d_act, None, d_red), -2, True, 0),
    ]


def _run_table(env, calls, column):
    """[(name, rc, named)] as observed, and the same from the table's literals."""
    seen, want = [], []
    for name, call, rc_in, named_in, rc_after in calls:
        exp = (rc_in, named_in) if column == 'in flight' else (rc_after, False)
        if exp[0] is None:
            continue
        rc = int(call())
        text = env.lib.cc4_last_error(env._h) or b''
        named = rc != 0 and text.startswith(name.encode() + b':')
        seen.append((name, rc, named if column == 'in flight' else False))
        want.append((name, exp[0], exp[1]))
        if column == 'in flight' and rc == -1 and not named:
            assert text == b'a rollout is in flight on this handle: cc4_rollout_end first', (name, text)
        if column == 'in flight' and named and name not in ('cc4_set_rng_state', 'cc4_replay_logged', 'cc4_allgather_obs'):
            assert b'a rollout is in flight' in text, (name, text)
    return seen, want


def test_refusals_with_a_rollout_in_flight_then_the_same_calls_succeed():
    from cage_challenge_4_amd import CC4VecEnv
    n, K = 6656, 1                      # K: the smallest rollout cc4_rollout_begin accepts
    small = CC4VecEnv(64, steps=50, rng_mode=1, autoreset=True, strict=False)
    small.reset(seeds=1)
    assert small.lib.cc4_rollout_begin(small._h, K) == -2 and b'no persistent kernel' in small.lib.cc4_last_error(small._h)      # (see the module's docstring)
    small.close()
    env = CC4VecEnv(n, steps=50, rng_mode=1, autoreset=True, strict=False)
    env.reset(seeds=11)
    sc = Scratch(16 << 20)
    try:
        lib, h = env.lib, env._h
        calls = _calls(env, sc)
        assert lib.cc4_rollout_begin(h, 0) == -2 and lib.cc4_rollout_begin(h, K) == 0, lib.cc4_last_error(h)
        seen, want = _run_table(env, calls, 'in flight')
        print('\n'.join(f'{s[0]:34s} rc {s[1]:2d} named {s[2]}' for s in seen))
        G, blk = ctypes.c_int32(), ctypes.c_int32()
        rc = lib.cc4_rollout_groups(h, ctypes.byref(G), ctypes.byref(blk))
        for g in range(G.value):
            rc = rc or lib.cc4_rollout_sync(h, -1, -1, g, 0, None)
            rc = rc or lib.cc4_rollout_random_policy(h, g, 0, ctypes.c_uint64(11), ctypes.c_uint32(0), None)
        for g in range(G.value):
            rc = rc or lib.cc4_rollout_sync(h, g, K - 1, -1, 0, None)
        assert lib.cc4_rollout_end(h) == 0 and rc == 0, lib.cc4_last_error(h)
        assert seen == want, [(s, w) for s, w in zip(seen, want) if s != w]
        seen, want = _run_table(env, calls, 'after')
        assert lib.cc4_synchronize(h) == 0
        assert seen == want, [(s, w, ) for s, w in zip(seen, want) if s != w]
    finally:
        env.close()
        sc.free()


def test_refusals_on_a_handle_with_a_communicator():
    from cage_challenge_4_amd import CC4VecEnv
    env = CC4VecEnv(4, steps=50, rng_mode=1, strict=False)
    env.reset(seeds=5)
    os.environ.setdefault('NCCL_SOCKET_IFNAME', 'lo')
    ident = (ctypes.c_uint8 * 128)()
    assert env.lib.cc4_comm_unique_id(ident) == 0
    env._chk(env.lib.cc4_comm_init(env._h, 0, 1, ident), 'cc4_comm_init')
    sc = Scratch(1 << 16)
    try:
        lib, h = env.lib, env._h
        d = sc.take(4096)
        seen = []
        for name, call in (('cc4_reset_device', lambda: lib.cc4_reset_device(h, None, None)),
                           ('cc4_step_red_device', lambda: lib.cc4_step_red_device(h, None, None, d)),
                           ('cc4_copy_episodes_device', lambda: lib.cc4_copy_episodes_device(h, 1, None, 0, d, None, 0, d, None)),
                           ('cc4_run_plan_device', lambda: lib.cc4_run_plan_device(h, 1, d, None, None, None, None))):
            rc = call()
            text = lib.cc4_last_error(h)
            seen.append((name, rc, text.startswith(name.encode() + b': not on a handle with a communicator')))
        assert seen == [(name, -2, True) for name, _, _ in seen], seen
        env.step(np.zeros((4, 5), np.int32))
    finally:
        env.close()
        sc.free()


@pytest.mark.parametrize('mode', ['enqueue-threads', 'one-thread', 'communicator'])
def test_group_streams_follow_the_main_stream(mode, monkeypatch):
    """Every former copy of the fork on one handle, main-stream work in between: launch_step (cc4_step_device in a loop, cc4_step behind an upload),
    group_prologue (cc4_step_group_device), run_threaded_groups (cc4_run_random_steps with the enqueue threads) and run_per_step (without them; its
    own fork, in front of a timed chunk's first event, is taken only where the launches cannot carry the timing events: with a communicator).
    CC4_MULTISTEP=0 and CC4_RUN1=0 keep the per-step launches for calls of 3 and of 12 steps: 64 episodes would be one launch otherwise."""
    monkeypatch.setenv('CC4_GROUPS', '3')
    monkeypatch.setenv('CC4_MULTISTEP', '0')
    monkeypatch.setenv('CC4_RUN1', '0')
    monkeypatch.setenv('CC4_ENQ_THREADS', '1' if mode == 'enqueue-threads' else '0')
    n, seed = 64, 404
    p = Pair(n, steps=40, rng_mode=1, seed0=seed)
    comm = mode == 'communicator'
    if comm:
        os.environ.setdefault('NCCL_SOCKET_IFNAME', 'lo')
        ident = (ctypes.c_uint8 * 128)()
        assert p.dev.lib.cc4_comm_unique_id(ident) == 0
        p.dev._chk(p.dev.lib.cc4_comm_init(p.dev._h, 0, 1, ident), 'cc4_comm_init')
    assert p.dev.launches_per_step == 3 and p.dev.run_kernel_for(12) == p.dev.step_kernel

    def clone():
        src, dst = np.array([3, 40]), np.array([22, 63])          # across the groups' boundaries (21 | 42)
        p.dev.clone_episodes(src, dst)
        for s, d in zip(src, dst):
            p.ora.restore(int(d), p.ora.snapshot(int(s)))
            p.ora._obs[d], p.ora._rew[d], p.ora._done[d], p.ora._err[d] = p.ora._obs[s], p.ora._rew[s], p.ora._done[s], p.ora._err[s]

    def timed(k):
        ms = p.dev.run_random_steps(seed, p.t, k, timed=True)
        assert ms > 0.0
        p._oracle_random(seed, k)

    def host_step():
        p.step(random_actions(seed, p.t, n))
        p.t += 1

    seq = [('cc4_step_device x2', lambda: p.policy_steps(seed, 2)),
           ('cc4_set_policies', lambda: p.dev.set_policies(red=-1, green=-1, blue=-1)),
           ('cc4_step_group_device x2', lambda: p.policy_steps(seed, 2, grouped=True)),
           ('run_random_steps 3', lambda: p.random_steps(seed, 3)),
           ('cc4_step_group_device', lambda: p.policy_steps(seed, 1, grouped=True)),
           ('run_random_steps 12', lambda: p.random_steps(seed, 12)),
           ('run_random_steps 3 timed', lambda: timed(3)),
           ('clone', clone),
           ('run_random_steps 12 timed', lambda: timed(12)),
           ('cc4_step_device', lambda: p.policy_steps(seed, 1)),
           ('clone', clone),
           ('run_random_steps 3', lambda: p.random_steps(seed, 3)),
           ('cc4_step', host_step),
           ('cc4_step_group_device', lambda: p.policy_steps(seed, 1, grouped=True)),
           ('masked reset', lambda: p.masked_reset(np.arange(n) % 5 == 0, np.arange(7000, 7000 + n, dtype=np.uint64))),
           ('run_random_steps 30 timed', lambda: timed(30)),
           ('cc4_step', host_step)]
    if comm:       # (group-wise stepping and episode copies refuse a handle with a communicator)
        seq = [c for c in seq if c[0] != 'clone' and 'group' not in c[0]]
    prev = 'reset'
    for i, (label, call) in enumerate(seq):
        call()
        bad = p.bad_outputs()
        assert bad.size == 0, _fail(i, prev, label, 'outputs', bad)
        what, bad = p.bad_rows(cold_every=7)
        assert what is None, _fail(i, prev, label, what, bad)
        prev = label
    p.close()


# ------------------------------------------------------------------------------------------------------------------------------------------
def _live(lib):
    out = (ctypes.c_int64 * 4)()
    assert lib.cc4_debug_live_resources(out) == 0
    return tuple(out)


def _touch_every_lazy_allocation(monkeypatch):
    """Three handles through every call that allocates on first use; returns the counts while they live.  64 episodes (counter mode) and 8 (a small
    handle: its inputs and outputs are pinned host memory, and cc4_keep_previous serves 16 episodes at the most) take everything but the persistent
    kernel; that, the rollout and the self-check's shadow handle need the batch tests/test_self_check_fires.py runs them at."""
    from cage_challenge_4_amd import CC4VecEnv
    from test_self_check_fires import N_PHILOX1, STEPS, K
    monkeypatch.delenv('CC4_PERSIST_VERIFY', raising=False)
    a = CC4VecEnv(64, steps=STEPS, rng_mode=1, autoreset=True, strict=False)
    b = CC4VecEnv(8, steps=STEPS, rng_mode=1, strict=False)
    monkeypatch.setenv('CC4_PERSIST_VERIFY', '1')
    c = CC4VecEnv(N_PHILOX1, steps=STEPS, rng_mode=1, autoreset=True, strict=False)
    lib = a.lib
    a.reset(seeds=1), b.reset(seeds=2), c.reset(seeds=3)
    # 64 episodes
    red = a.agent_actions('red')
    red['type'][0, 0] = 9                                         # one record: Sleep
    a.step_ex(random_actions(1, 0, 64), red=red)                  # d_ext
    a.set_policies(red=-1)                                        # d_pol
    a.policies()
    a.clone_episodes([3], [4], seeds=[77])                        # d_copy_idx, d_copy_seeds
    a.enable_reward_terms(True)
    a.debug_digest()                                              # d_digest
    a.run_plan(np.zeros((2, 64, 5), np.int32))                    # d_plan_err
    assert a.run_random_steps(1, 1, 3, timed=True) > 0.0          # the timing events
    a.step(random_actions(1, 4, 64))                              # the pinned staging blocks of a batch that is not small
    assert lib.cc4_debug_profile(a._h, 1, None) == 0              # d_prof, left enabled
    # 8 episodes
    b.keep_previous(True)                                         # d_prev_*
    b.step(random_actions(2, 0, 8))
    b.replay_logged()
    assert lib.cc4_debug_profile(b._h, 1, None) == 0
    # the persistent kernel's batch, every call checked against a shadow handle
    assert c.run_kernel_for(K) == 'k_run_philox1'                 # persist_setup: d_pool, d_slot_part, d_run, the shadow handle
    c.run_rollout(2, 'random', 3, 0)                              # d_ract .. d_rfail, the policy streams, d_xslab, the watchdog word
    c.run_random_steps(3, 2, K, timed=True)                       # a checked call: both handles' d_digest
    c.run_plan(np.zeros((K, N_PHILOX1, 5), np.int32), record_obs=True)      # a checked plan call: the shadow's trajectory, call-local
    assert c.verify_stats() == (2, 0)
    sh = VP()
    assert lib.cc4_debug_shadow_handle(c._h, ctypes.byref(sh)) == 0 and sh.value
    assert lib.cc4_debug_profile(c._h, 1, None) == 0
    live = _live(lib)
    for env in (a, b, c):
        env.close()
    return live


def test_resources_return_to_baseline(monkeypatch):
    import gc
    from cage_challenge_4_amd import _lib
    lib = _lib.load()
    gc.collect()                       # (handles an earlier test of this process dropped without closing them)
    base = _live(lib)
    for cycle in range(2):
        live = _touch_every_lazy_allocation(monkeypatch)
        assert all(x > y for x, y in zip(live, base)), (cycle, live, base)
        assert _live(lib) == base, (cycle, live)
