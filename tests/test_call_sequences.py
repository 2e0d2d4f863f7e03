"""One handle driven through every way of stepping it, in turn, against the CPU oracle: host steps, device-action steps (whole batch and per
group), short run_random_steps calls (per-step launches), one-launch persistent calls (k_run_philox1 / k_run_pcg), rollouts with the policy in
the loop (k_run_philox1r), masked resets, snapshot restores and reseeds -- what a training loop does between its rollouts.  The persistent
schedule keeps state on the handle from one call to the next (two parities of ticket lines, progress words counted since they were last
cleared); the tests elsewhere run each form back to back only.  After every call the outputs (observations, rewards, dones, error words), and
every few calls and at the end the generator positions, every hot row and sampled cold rows, are compared with the oracle."""
import ctypes

import numpy as np
import pytest
from oracle_binding import OracleVecEnv, random_actions
from rollout_util import hash_policy, pack_rows

pytestmark = pytest.mark.gpu

WRAP = 0x700000          # persist_launch clears the progress words when a call would take them past this many steps (csrc/cc4_api_run.hip)
RING = 32                # slabs of packed observation rows a rollout keeps (cc4_rollout_obs_packed)


class Pair:
    """A device handle and the oracle, moved by the same calls.  `t` is the action time of the next random draw."""

    def __init__(self, n, steps, rng_mode, seed0):
        from cage_challenge_4_amd import CC4VecEnv
        self.n, self.rng_mode = n, rng_mode
        self.dev = CC4VecEnv(n, steps=steps, rng_mode=rng_mode, autoreset=True, strict=False)
        self.ora = OracleVecEnv(n, steps=steps, rng_mode=rng_mode, autoreset=True)
        o = self.ora.reset_batch(seed0)
        d = self.dev.reset(seeds=seed0)
        assert np.array_equal(d, o), 'observations of the first reset'
        assert np.array_equal(self.dev.action_mask, self.ora.mask()), 'action masks of the first reset'
        self.t = 0
        self.sb = int(self.dev.lib.cc4_state_bytes())

    def close(self):
        self.dev.close()
        self.ora.close()

    # ---- what is compared
    def bad_outputs(self, skip=()):
        """Episodes whose observations, reward, done or error word differ (the handle's outputs of its last stepping call or reset), but for `skip`."""
        d, o = self.dev, self.ora
        d.synchronize()
        d._fetch()
        bad = (d._obs != o._obs).any(axis=1) | (d._rew != o._rew) | (d._done.astype(bool) != o._done) | (d._err != o._err)
        bad[list(skip)] = False
        return np.nonzero(bad)[0]

    def ora_states(self):
        p0 = self.ora.lib.cc4o_state_ptr(self.ora._h, 0)
        if self.n > 1 and self.ora.lib.cc4o_state_ptr(self.ora._h, self.n - 1) - p0 == (self.n - 1) * self.sb:     # (one array: one copy)
            return np.frombuffer((ctypes.c_uint8 * (self.n * self.sb)).from_address(p0), np.uint8).reshape(self.n, self.sb).copy()
        return np.stack([self.ora.get_state(i) for i in range(self.n)])

    def bad_rows(self, envs=None, cold_every=61):
        """(what, episodes) of the first kind of row that differs: generator positions, hot rows (all episodes, or `envs`), cold rows (every
        cold_every-th episode and `envs`)."""
        d, o = self.dev, self.ora
        bad = np.nonzero((d.rng_state() != o.rng_state()).any(axis=1))[0]
        if bad.size:
            return 'generator state', bad
        if envs is None:
            bad = np.nonzero((d.get_states() != self.ora_states()).any(axis=1))[0]
        else:
            bad = np.array([i for i in envs if not np.array_equal(d.get_state(i), o.get_state(i))], int)
        if bad.size:
            return 'hot row', bad
        cold = sorted(set(range(0, self.n, cold_every)) | set(envs if envs is not None else []))
        bad = np.array([i for i in cold if not np.array_equal(d.get_cold(i), o.get_cold(i))], int)
        if bad.size:
            return 'cold row', bad
        return None, bad

    # ---- the calls
    def step(self, a, m=None):
        self.dev.step(a, m)
        self.ora.step_batch(a, m)

    def random_steps(self, seed, k):
        """cc4_run_random_steps: per-step launches below persist_min_k steps, one launch of the persistent kernel from there on."""
        self.dev.run_random_steps(seed, self.t, k, timed=False)
        self._oracle_random(seed, k)

    def policy_steps(self, seed, k, grouped=False):
        (self.dev.run_policy_steps_grouped if grouped else self.dev.run_policy_steps)(seed, self.t, k)
        self._oracle_random(seed, k)

    def _oracle_random(self, seed, k):
        for i in range(k):
            self.ora.step_batch(random_actions(seed, self.t + i, self.n))
        self.t += k

    def rollout(self, k, policy, seed, native):
        """A k-step rollout; returns the packed rows the policy of each step read, as the oracle has them ([k] of [n, 148])."""
        self.dev.run_rollout(k, policy, seed, self.t, native=native)
        read = []
        for j in range(k):
            rows = pack_rows(self.ora._obs)
            read.append(rows if j >= k - (RING - 1) else None)     # (the ring holds the last 31 of them)
            self.ora.step_batch(random_actions(seed, self.t + j, self.n) if policy == 'random' else hash_policy(rows, j))
        self.t += k
        return read

    def masked_reset(self, mask, seeds):
        self.dev.reset(seeds=seeds, env_mask=mask.astype(np.uint8))
        self.ora.reset(seeds=seeds, env_mask=mask)
        sel = np.nonzero(mask)[0]
        want = np.zeros((sel.size, 570), np.uint8)
        for r, i in enumerate(sel):
            self.ora.lib.cc4o_mask(self.ora._h, int(i), want[r].ctypes.data_as(ctypes.c_void_p))
        # (the handle's mask is written by cc4_reset only, and only for the episodes it regenerated)
        return sel[(self.dev.action_mask[sel] != want.astype(bool)).any(axis=1)]


def _fail(i, prev, kind, what, bad):
    return f'call {i} ({prev} -> {kind}): {what} differ(s), first bad episodes {bad[:8].tolist()} of {bad.size}'


# ------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('n', [6656, 8192])
@pytest.mark.parametrize('groups', [1, 2, 3, 4])
def test_rollouts_and_one_launch_calls_alternate(groups, n, monkeypatch):
    """Rollouts and one-launch calls in turn.  A rollout counts tickets in words 0 .. G-1 of its parity's lines, a one-launch call in word 0; a
    rollout behind an odd number of one-launch calls finds the lines of the rollout before it -- with a smaller k its groups 1 .. G-1 looked
    handed out (-6 with half the batch stepped), with a larger k the first tickets named steps the progress words never reach (the kernel
    spun for good).  The smaller-k rollout comes first, so that a tree with that bug fails on -6 before it reaches the case that hangs."""
    monkeypatch.setenv('CC4_ROLLOUT_GROUPS', str(groups))
    monkeypatch.setenv('CC4_ROLLOUT_WATCHDOG_MS', '500')
    seed = 5150 + groups + n
    p = Pair(n, steps=55, rng_mode=1, seed0=seed)
    assert p.dev.run_kernel_for(10) == 'k_run_philox1' and p.dev.run_kernel_for(9) == p.dev.step_kernel
    seq = [('rollout', 20), ('call', 10), ('rollout', 12), ('call', 13), ('call', 11), ('call', 16), ('rollout', 31), ('call', 10),
           ('call', 14), ('rollout', 25), ('short', 6), ('rollout', 8)]
    prev = 'reset'
    for i, (kind, k) in enumerate(seq):
        if kind == 'rollout':
            p.rollout(k, 'hash' if i % 4 else 'random', seed + i, native=(i % 3 == 0))
        else:
            p.random_steps(seed + i, k)
        label = f'{kind} k={k}'
        bad = p.bad_outputs()
        assert bad.size == 0, _fail(i, prev, label, 'outputs', bad)
        if i % 4 == 3 or i == len(seq) - 1:
            what, bad = p.bad_rows()
            assert what is None, _fail(i, prev, label, what, bad)
        prev = label
    G, blk = ctypes.c_int32(), ctypes.c_int32()
    assert p.dev.lib.cc4_rollout_groups(p.dev._h, ctypes.byref(G), ctypes.byref(blk)) == 0 and G.value == groups
    p.close()


# ------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('K', [1, 2, 32, 33, 100])
def test_rollout_lengths_at_the_edges_of_the_ring(K):
    """A rollout keeps the packed rows of its last 32 steps in a ring of slabs; the 'hash' policy computes its actions from the rows it reads, so a
    stale or early slab changes the trajectory.  Rollouts of 1, 2, 32, 33 and 100 steps, enqueued from Python and by cc4_rollout_standin, one
    behind the other on one handle; after each, the rows cc4_rollout_obs_packed gives for its last 31 steps against the oracle's."""
    n, seed = 8192, 606 + K
    p = Pair(n, steps=50, rng_mode=1, seed0=seed)
    prev = 'reset'
    for i, native in enumerate((False, True)):
        read = p.rollout(K, 'hash', seed, native=native)
        label = f'rollout K={K} ' + ('native' if native else 'python')
        bad = p.bad_outputs()
        assert bad.size == 0, _fail(i, prev, label, 'outputs', bad)
        for j in range(max(0, K - (RING - 1)), K):
            got = p.dev.rollout_obs_packed(j)
            bad = np.nonzero((got != read[j]).any(axis=1))[0]
            assert bad.size == 0, _fail(i, prev, label, f'packed rows policy step {j} read', bad)
        prev = label
    what, bad = p.bad_rows()
    assert what is None, _fail(1, 'rollout', prev, what, bad)
    p.close()


# ------------------------------------------------------------------------------------------------------------------------------------------
def de_bruijn_pairs(m):
    """A de Bruijn sequence B(m, 2), made linear: m * m + 1 symbols of 0 .. m-1 in which every ordered pair (a, b) follows each other once."""
    a, seq = [0] * (2 * m), []

    def db(t, q):
        if t > 2:
            if 2 % q == 0:
                seq.extend(a[1:q + 1])
        else:
            a[t] = a[t - q]
            db(t + 1, q)
            for v in range(a[t - q] + 1, m):
                a[t] = v
                db(t + 1, t)
    db(1, 1)
    return seq + seq[:1]


KINDS = ['step', 'step+messages', 'policy_steps', 'policy_steps_grouped', 'random_steps 1-9', 'random_steps 10-40', 'random_steps 64-90',
         'rollout random', 'rollout hash', 'masked reset', 'restore', 'set_seed']


@pytest.mark.parametrize('rng_mode,n', [(1, 8192), (0, 5000)], ids=['counter', 'numpy-stream'])
def test_every_ordered_pair_of_call_kinds(rng_mode, n):
    """One handle through a de Bruijn sequence of call kinds: every kind follows every kind (itself included) once, each call's parameters from a
    fixed-seed generator.  The numpy-stream handle (k_run_pcg) has no rollouts.  Host steps with messages come before the one-launch calls,
    which skip the message encode after a call's first step; restores and reseeds write rows that the next call must pick up."""
    kinds = KINDS if rng_mode == 1 else [k for k in KINDS if not k.startswith('rollout')]
    order = de_bruijn_pairs(len(kinds))
    pairs = {(order[i], order[i + 1]) for i in range(len(order) - 1)}
    assert len(pairs) == len(kinds) ** 2, 'every ordered pair of call kinds occurs'
    rng = np.random.default_rng(4242 + rng_mode)
    seed = 9000 + rng_mode
    p = Pair(n, steps=50, rng_mode=rng_mode, seed0=seed)
    run1 = 'k_run_philox1' if rng_mode == 1 else 'k_run_pcg'
    assert p.dev.run_kernel_for(10) == run1 and p.dev.run_kernel_for(9) == p.dev.step_kernel
    snaps = {}

    def take_snapshots(count):
        for e in rng.choice(n, count, replace=False):
            e = int(e)
            s = p.dev.snapshot(e)
            assert np.array_equal(s[0], p.ora.get_state(e)) and np.array_equal(s[1], p.ora.get_cold(e)), ('snapshot', e)
            snaps[e] = s

    take_snapshots(3)
    prev, since_rows = 'reset', 0
    stale = set()              # restored episodes whose outputs the handle has not rewritten yet (the oracle's restore sets their done flag)
    for i, c in enumerate(order):
        kind = kinds[c]
        s = int(rng.integers(1, 1 << 31))
        label = kind
        touched = None
        if kind == 'step':
            p.step(random_actions(s, p.t, n)); p.t += 1
        elif kind == 'step+messages':
            p.step(random_actions(s, p.t, n), rng.integers(0, 2, size=(n, 5, 8)).astype(np.uint8)); p.t += 1
        elif kind.startswith('policy_steps'):
            k = int(rng.integers(1, 4)); label += f' k={k}'
            p.policy_steps(s, k, grouped=kind.endswith('grouped'))
        elif kind.startswith('random_steps'):
            lo, hi = {'1-9': (1, 9), '10-40': (10, 40), '64-90': (64, 90)}[kind.split()[1]]
            k = int(rng.integers(lo, hi + 1)); label += f' k={k}'
            p.random_steps(s, k)
        elif kind.startswith('rollout'):
            k, native = int(rng.integers(1, 41)), bool(rng.integers(0, 2)); label += f' k={k}' + (' native' if native else '')
            p.rollout(k, kind.split()[1], s, native)
        elif kind == 'masked reset':
            mask = rng.random(n) < 0.05
            mask[int(rng.integers(0, n))] = True
            seeds = rng.integers(1, 1 << 40, n).astype(np.uint64)
            bad = p.masked_reset(mask, seeds)
            assert bad.size == 0, _fail(i, prev, label, 'action masks of the reset episodes', bad)
            touched = np.nonzero(mask)[0][:16]
            stale -= set(np.nonzero(mask)[0].tolist())
        elif kind == 'restore':
            # every episode with a snapshot goes back to it (taken at an earlier restore, or at the start); then snapshots of others for later
            touched = np.array(sorted(snaps), int)
            stale |= set(snaps)
            for e, snap in snaps.items():
                p.dev.restore(e, snap)
                p.ora.restore(e, snap)
            snaps.clear()
            take_snapshots(3)
        elif kind == 'set_seed':
            seeds = rng.integers(1, 1 << 40, n).astype(np.uint64)
            p.dev.set_seed(seeds)
            p.ora.set_seed(seeds)
            touched = np.arange(0, n, 97)
        if kind not in ('restore', 'set_seed'):
            # (a restore or a reseed writes no outputs: what they wrote shows in the next stepping call's outputs -- a restored episode's
            # observation buffer holds the previous occupant's values until then)
            bad = p.bad_outputs(skip=stale if kind == 'masked reset' else ())
            assert bad.size == 0, _fail(i, prev, label, 'outputs', bad)
            if kind != 'masked reset':
                stale.clear()
        if touched is not None:
            what, bad = p.bad_rows(envs=touched.tolist())
            assert what is None, _fail(i, prev, label, what, bad)
        since_rows += 1
        if since_rows >= 8 or i == len(order) - 1:
            what, bad = p.bad_rows()
            assert what is None, _fail(i, prev, label, what, bad)
            since_rows = 0
        prev = label
    p.close()


# ------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('rng_mode,n', [(1, 8192), (0, 5000)], ids=['counter', 'numpy-stream'])
def test_progress_words_wrap(rng_mode, n):
    """The persistent schedule's progress words count steps since they were last cleared, and persist_launch clears them when a call would take
    them past 0x700000 -- some 7.3 M batch steps, minutes of a real run, never reached by a test without the hook that puts them there.  A call
    that ends exactly at the mark (no wrap), one that crosses it, and in the counter mode a rollout across it."""
    seed = 777 + rng_mode
    p = Pair(n, steps=45, rng_mode=rng_mode, seed0=seed)
    lib, h = p.dev.lib, p.dev._h
    run1 = 'k_run_philox1' if rng_mode == 1 else 'k_run_pcg'
    assert p.dev.run_kernel_for(10) == run1
    assert lib.cc4_debug_persist_base(h, WRAP + 1) == -2
    p.random_steps(seed, 5)                                         # (a few plain steps first: the words are not where a fresh handle has them)
    seq = [('base', WRAP - 12), ('call', 12), ('call', 10), ('call', 21)]
    if rng_mode == 1:
        seq += [('base', WRAP - 5), ('rollout', 20), ('call', 11)]
    prev = 'reset'
    for i, (kind, v) in enumerate(seq):
        label = f'{kind} {v:#x}' if kind == 'base' else f'{kind} k={v}'
        if kind == 'base':
            assert lib.cc4_debug_persist_base(h, v) == 0, lib.cc4_last_error(h)
        elif kind == 'call':
            p.random_steps(seed + i, v)
        else:
            p.rollout(v, 'hash', seed + i, native=False)
        if kind != 'base':
            bad = p.bad_outputs()
            assert bad.size == 0, _fail(i, prev, label, 'outputs', bad)
        prev = label
    what, bad = p.bad_rows()
    assert what is None, _fail(len(seq) - 1, 'call', prev, what, bad)
    p.close()


# ------------------------------------------------------------------------------------------------------------------------------------------
def test_rollout_policy_calls_check_their_ranges(monkeypatch):
    """cc4_rollout_random_policy / cc4_rollout_hash_policy take g in 0 .. G-1 and j in 0 .. k-1, cc4_rollout_obs_packed j >= 0: anything else is -2
    and launches nothing.  (The values used here name streams and memory that exist: without the checks the calls would write an action slot of
    the rollout in flight -- the comparison with the oracle below fails, nothing faults.)  Then the rollout is finished as usual."""
    monkeypatch.setenv('CC4_ROLLOUT_GROUPS', '2')
    n, K, seed = 8192, 6, 31
    p = Pair(n, steps=50, rng_mode=1, seed0=seed)
    lib, h = p.dev.lib, p.dev._h
    assert lib.cc4_rollout_begin(h, K) == 0, lib.cc4_last_error(h)
    s0 = ctypes.c_uint64(seed)
    for g, j in ((2, 0), (3, 0), (0, -1), (1, K)):
        assert lib.cc4_rollout_random_policy(h, g, j, s0, ctypes.c_uint32(0), None) == -2, (g, j)
        assert b'out of range' in lib.cc4_last_error(h)
        assert lib.cc4_rollout_hash_policy(h, g, j, None) == -2, (g, j)
    rows = ctypes.c_void_p()
    assert lib.cc4_rollout_obs_packed(h, -1, ctypes.byref(rows)) == -2
    assert lib.cc4_debug_persist_base(h, 0) == -2 and b'in flight' in lib.cc4_last_error(h)
    rc = 0
    for j in range(K):
        for g in range(2):
            rc = rc or lib.cc4_rollout_sync(h, g if j > 0 else -1, j - 1, g, j, None)
            rc = rc or lib.cc4_rollout_random_policy(h, g, j, s0, ctypes.c_uint32(j), None)
    for g in range(2):
        rc = rc or lib.cc4_rollout_sync(h, g, K - 1, -1, 0, None)
    assert lib.cc4_rollout_end(h) == 0 and rc == 0, lib.cc4_last_error(h)
    p._oracle_random(seed, K)
    bad = p.bad_outputs()
    assert bad.size == 0, _fail(0, 'reset', f'rollout K={K}', 'outputs', bad)
    what, bad = p.bad_rows()
    assert what is None, _fail(0, 'reset', f'rollout K={K}', what, bad)
    p.close()
