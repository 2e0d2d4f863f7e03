"""GPU: the self-check can fail.  Every `verify_stats() == (calls, 0)` of this suite draws its conclusion from a zero that k_digest, the host's
compare and -- for plan calls -- the trajectory compare produce; here that instrument is held against a reference of its own and shown reporting
differences that are known to be there.  Every comparison is exact.

* k_digest == cc4_debug_digest_rows (csrc/cc4_digest.h compiled for the host) == tests/digest_util.py (numpy, from the prose of include/cc4_debug.h)
  on the rows of real handles behind the three step kernels.
* One launch of k_digest over 256 equal episodes each of which has ONE bit flipped in another 16-byte vector of its hot (then cold) row: 256 distinct
  words, every one off the clean word, the other two words untouched.
* cc4_debug_verify_plant: one byte of the SHADOW's side changed between the runs and the compare -- data only, never stepped, never on the main handle.
  A checked call of every self-checked kernel then returns -5, counts a mismatch, names the kernel, the episode and exactly the planted part; the call
  behind it is clean; and the main handle ends where the oracle ends, so a reported mismatch leaves the batch intact.
* Plan calls: a planted reward / done / packed byte of the shadow's recorded trajectory is placed at its step and episode.
* The sampled default (CC4_PERSIST_VERIFY_EVERY) reports the plant at the call it checks; refusals leave nothing armed."""
import ctypes
import os
import re

import numpy as np
import pytest

import digest_util as D
import handover_util as H
from oracle_binding import OracleVecEnv, random_actions
from plan_util import random_plan

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STEPS = 40                    # short episodes: small cold rows, regenerations inside every call sequence
K = 12
N_PHILOX1 = 5121              # the smallest batches whose calls take the persistent kernels (asserted: one episode fewer takes another kernel)
N_PCG = 3073
RUN_LONG_K = int(re.search(r'\bRUN_LONG_K = (\d+)', open(os.path.join(ROOT, 'cage_challenge_4_amd', 'csrc', 'cc4_sched.h')).read()).group(1))
PART_NAMES = {0: 'hot row', 1: 'cold row', 2: 'outputs', 3: 'outputs', 4: 'outputs', 5: 'outputs', 6: 'outputs'}
TRAJ_NAMES = {7: 'rewards', 8: 'dones', 9: 'packed observations'}
VERIFY_ENV = ('CC4_PERSIST_VERIFY', 'CC4_PERSIST_VERIFY_EVERY', 'CC4_PERSIST_THR', 'CC4_PERSIST_RUNS', 'CC4_PERSIST', 'CC4_PERSIST_MIN_K', 'CC4_PHILOX_LEAN', 'CC4_MULTISTEP', 'CC4_RUN1')


def _dev(n, **kw):
    from cage_challenge_4_amd import CC4VecEnv
    return CC4VecEnv(n, steps=STEPS, autoreset=True, strict=False, **kw)


def _clean_env(monkeypatch, **setenv):
    for k in VERIFY_ENV:
        monkeypatch.delenv(k, raising=False)
    for k, v in setenv.items():
        monkeypatch.setenv(k, v)


def _set_cold(dev, e, cold):
    cold = np.ascontiguousarray(cold, dtype=np.uint8)
    assert cold.size == dev.lib.cc4_cold_bytes(dev._h)
    dev._chk(dev.lib.cc4_set_cold(dev._h, int(e), cold.ctypes.data_as(ctypes.c_void_p)), 'cc4_set_cold')


def _outputs(dev):
    """(obs, reward, done, err, actions) of every episode as the handle's device buffers hold them."""
    dev.synchronize()
    dev._chk(dev.lib.cc4_fetch(dev._h, *dev._p_out), 'cc4_fetch')
    return dev._obs.copy(), dev._rew.copy(), dev._done.copy(), dev._err.copy(), dev.device_actions()


# ------------------------------------------------------------------------------------------------ kernel == host function == restatement
@pytest.mark.parametrize('n', [5, 65])
@pytest.mark.parametrize('kernel,rng_mode,lean', [('k_step', 0, None), ('k_step_philox', 1, '0'), ('k_step_philox1', 1, '1')])
def test_kernel_equals_host_function_and_restatement(kernel, rng_mode, lean, n, monkeypatch):
    _clean_env(monkeypatch, **({} if lean is None else {'CC4_PHILOX_LEAN': lean}))
    dev = _dev(n, rng_mode=rng_mode)
    assert dev.step_kernel == kernel
    dev.reset(seeds=300)
    for t in range(25):
        dev.step(random_actions(300, t, n))
    got = dev.debug_digest()
    assert got.shape == (n, 3) and got.dtype == np.uint64
    hot, (obs, rew, done, err, act) = dev.get_states(), _outputs(dev)
    assert done.dtype == np.uint8 and obs.dtype == np.int32 and obs.any() and rew.any()
    for e in range(n):
        ep = (hot[e], dev.get_cold(e), obs[e], float(rew[e]), int(done[e]), int(err[e]), act[e])
        host, num = D.host_digest(*ep), D.digest(*ep)
        assert np.array_equal(got[e], host), (kernel, n, e, [hex(int(v)) for v in got[e]], [hex(int(v)) for v in host])
        assert np.array_equal(host, num), (kernel, n, e)
    assert len({int(v) for v in got.reshape(-1)}) == 3 * n          # different episodes, different words
    assert np.array_equal(dev.debug_digest(), got) and np.array_equal(dev.get_states(), hot)       # read-only
    dev.close()


# ------------------------------------------------------------------------------------------------ kernel sensitivity in one launch
def _positions(nv):
    """The vector indices the flips cover: the first round 0..63, the first vector of the second round, the last 64 (every lane's last vector)."""
    assert nv > 3 * D.LANES
    return list(range(D.LANES)) + [D.LANES] + list(range(nv - D.LANES, nv))


def test_one_launch_tells_256_single_bit_flips_apart(monkeypatch):
    _clean_env(monkeypatch)
    n = 256
    dev = _dev(n, rng_mode=0)
    dev.reset(seeds=np.full(n, 9, np.uint64))
    dev._chk(dev.lib.cc4_random_actions_device(dev._h, ctypes.c_uint64(9), ctypes.c_uint32(0)), 'cc4_random_actions_device')      # (the action buffer of a fresh handle holds nothing yet)
    clean = dev.debug_digest()
    assert (clean[:, :2] == clean[0, :2]).all(), 'one seed, equal rows, equal row words'
    hot0, cold0 = dev.get_state(0), dev.get_cold(0)
    assert all(np.array_equal(dev.get_state(e), hot0) for e in (1, 100, n - 1)) and np.array_equal(dev.get_cold(n - 1), cold0)
    obs, rew, done, err, act = _outputs(dev)
    assert np.array_equal(clean[0], D.host_digest(hot0, cold0, obs[0], float(rew[0]), int(done[0]), int(err[0]), act[0]))
    for which, row0, put in ((0, hot0, dev.set_state), (1, cold0, lambda e, r: _set_cold(dev, e, r))):
        pos = _positions(row0.size // 16)
        want = np.zeros(n, np.uint64)
        for e in range(n):                                  # episode e: vector pos[e % 129]; bit 0 of its first byte, then bit 7 of its last
            v, second = pos[e % len(pos)], e >= len(pos)
            r = row0.copy()
            r[16 * v + (15 if second else 0)] ^= 0x80 if second else 1
            put(e, r)
            want[e] = D.row_word(r)
        got = dev.debug_digest()
        other = [i for i in range(3) if i != which]
        assert np.array_equal(got[:, other], clean[:, other]), which
        assert (got[:, which] != clean[0, which]).all(), (which, np.nonzero(got[:, which] == clean[0, which])[0].tolist())
        assert len({int(v) for v in got[:, which]}) == n, which
        assert np.array_equal(got[:, which], want), (which, np.nonzero(got[:, which] != want)[0][:8].tolist())        # .. and they are the restatement's words
        for e in range(n):                                  # restored, never stepped while flipped
            put(e, row0)
        assert np.array_equal(dev.debug_digest(), clean), which
    dev.close()


# ------------------------------------------------------------------------------------------------ the check fires
def _plants(n, hot_bytes, cold_bytes):
    """(part, episode, offset): parts 0..6, episodes 0 / a middle one / n - 1, first and last byte of a row, first and last value."""
    mid = n // 2 + 1
    return [(0, 0, 0), (0, n - 1, hot_bytes - 1), (0, mid, hot_bytes // 2), (1, mid, 0), (1, 0, cold_bytes - 1), (1, n - 1, cold_bytes // 3),
            (2, n - 1, 0), (2, 0, D.OBS - 1), (3, mid, 0), (4, 0, 0), (5, n - 1, 0), (6, 0, 0), (6, mid, D.NBLUE - 1)]


def _parse(msg):
    """(episode, [parts named]) of a mismatch message's digest clause, or None."""
    m = re.search(r'first episode (\d+) \(([^)]*)\)', msg)
    return (int(m.group(1)), [p for p in ('hot row', 'cold row', 'outputs') if p in m.group(2)]) if m else None


def _same_as_oracle(dev, ora, want_out, want_actions, what):
    """The main handle against the oracle: observations, rewards, dones, err, the last actions, generator words, every hot row, a stride of cold rows."""
    obs, rew, done, err, act = _outputs(dev)
    o, r, d, info = want_out
    bad = np.nonzero((obs != o).any(axis=1) | (rew.view(np.uint32) != r.view(np.uint32)) | (done.astype(bool) != d) | (err != info['err']))[0]
    assert bad.size == 0, (what, 'outputs', bad[:8].tolist())
    assert np.array_equal(act, want_actions), (what, 'actions')
    assert np.array_equal(dev.rng_state(), ora.rng_state()), (what, 'generator words')
    n = dev.num_envs
    bad = np.nonzero((dev.get_states() != np.stack([ora.get_state(i) for i in range(n)])).any(axis=1))[0]
    assert bad.size == 0, (what, 'hot rows', bad[:8].tolist())
    for i in sorted(set(range(0, n, 512)) | {n - 1}):
        assert np.array_equal(dev.get_cold(i), ora.get_cold(i)), (what, 'cold row', i)


def _smaller_batch_takes_another_kernel(n, rng_mode, kernel, plan):
    dev = _dev(n - 1, rng_mode=rng_mode)
    other = dev.plan_kernel_for(K) if plan else dev.run_kernel_for(K)
    dev.close()
    assert other != kernel, (n - 1, other)


@pytest.mark.parametrize('kernel,n,rng_mode,long_call', [('k_run_philox', 64, 1, 0), ('k_run_philox1', N_PHILOX1, 1, RUN_LONG_K), ('k_run_pcg', N_PCG, 0, 0)])
def test_a_planted_difference_is_reported_and_the_batch_stays_intact(kernel, n, rng_mode, long_call, monkeypatch):
    from cage_challenge_4_amd._lib import CC4Error
    _clean_env(monkeypatch, CC4_PERSIST_VERIFY='1')
    if n > 64:
        _smaller_batch_takes_another_kernel(n, rng_mode, kernel, False)
    seed0 = 4100
    dev, ora = _dev(n, rng_mode=rng_mode), OracleVecEnv(n, steps=STEPS, rng_mode=rng_mode, autoreset=True)
    assert np.array_equal(dev.reset(seeds=seed0), ora.reset_batch(seed0))
    assert dev.run_kernel_for(K) == kernel and (not long_call or dev.run_kernel_for(long_call) == kernel)
    state = {'t': 0, 'out': None, 'act': None}

    def call(k=K):
        t = state['t']
        state['t'] = t + k
        for j in range(k):                                   # the oracle first: the main handle runs the call whether or not it is reported
            state['act'] = random_actions(seed0, t + j, n)
            state['out'] = ora.step_batch(state['act'])
        dev.run_random_steps(seed0, t, k, timed=False)

    def planted(part, e, off, k=K):
        calls, bad = dev.verify_stats()
        assert dev.debug_verify_plant(part, e, off) == 0, (part, e, off)
        with pytest.raises(CC4Error) as ei:
            call(k)
        msg = str(ei.value)
        assert 'rc=-5' in msg and f'CC4_PERSIST_VERIFY: {kernel} and the per-step launches disagree after {k} steps: first episode {e} (' in msg, msg
        assert _parse(msg) == (e, [PART_NAMES[part]]), (part, e, off, msg)
        assert dev.verify_stats() == (calls + 1, bad + 1), (part, e, off)

    call()
    assert dev.verify_stats() == (1, 0)
    plants = _plants(n, int(dev.lib.cc4_state_bytes()), int(dev.lib.cc4_cold_bytes(dev._h)))
    assert {p for p, _, _ in plants} == set(range(7)) and {e for _, e, _ in plants} == {0, n // 2 + 1, n - 1}
    planted(*plants[0])
    assert dev.verify_stats() == (2, 1)
    call()                                                   # the call behind a reported one is clean: nothing stayed armed, the shadow was re-seeded
    assert dev.verify_stats() == (3, 1)
    for p in plants[1:]:
        planted(*p)
    if long_call:
        planted(0, n - 1, 64, long_call)                     # one long call (runs of RUN_LONG_SA and a closing run)
    checked, bad = dev.verify_stats()
    call()
    assert dev.verify_stats() == (checked + 1, bad) and bad == len(plants) + (1 if long_call else 0)
    _same_as_oracle(dev, ora, state['out'], state['act'], kernel)
    assert not dev.err.any()
    dev.close(), ora.close()


@pytest.mark.parametrize('kernel,n,rng_mode', [('k_run_philox1p', N_PHILOX1, 1), ('k_run_pcgp', N_PCG, 0)])
def test_plan_calls_report_planted_digest_and_trajectory_differences(kernel, n, rng_mode, monkeypatch):
    _clean_env(monkeypatch, CC4_PERSIST_VERIFY='1')
    _smaller_batch_takes_another_kernel(n, rng_mode, kernel, True)
    dev, ora = _dev(n, rng_mode=rng_mode), OracleVecEnv(n, steps=STEPS, rng_mode=rng_mode, autoreset=True)
    assert np.array_equal(dev.reset(seeds=H.RESET_SEED), ora.reset_batch(H.RESET_SEED))
    assert dev.plan_kernel_for(K) == kernel
    rng = np.random.default_rng(n)
    state = {}

    def call(expect_rc=0):
        """One recorded plan call of K steps through the raw driver; the main side's recorded rows must be the oracle's whatever the call returns."""
        act, msg = random_plan(rng, K, n, True)
        if expect_rc == -2:                                  # a refused call steps nothing
            res = H.run_plan_raw(dev, act, msg, record_obs=True)
            assert res.rc == -2, (res.rc, res.error)
            return res
        rew, done, packed = np.zeros((K, n), np.float32), np.zeros((K, n), bool), np.zeros((K, n, H.OBS_PACKED), np.uint8)
        for j in range(K):
            state['out'] = o, r, d, _ = ora.step_batch(act[j], msg[j])
            rew[j], done[j], packed[j] = r, d, H.pack_obs(o)
        state['act'] = act[-1]
        res = H.run_plan_raw(dev, act, msg, record_obs=True)
        assert res.rc == expect_rc, (res.rc, res.error)
        assert np.array_equal(res.rewards.view(np.uint32), rew.view(np.uint32)) and np.array_equal(res.dones, done) and np.array_equal(res.obs_packed, packed)
        return res

    head = f'CC4_PERSIST_VERIFY: {kernel} and the per-step launches disagree after a plan of {K} steps: '
    call()
    assert dev.verify_stats() == (1, 0)
    mid = n // 2 + 1
    bad = 0
    # the digest's parts on a plan call: named, and no trajectory row differs
    for part, e, off in ((0, mid, 17), (1, n - 1, 0), (2, 0, 3), (3, n - 1, 0), (4, mid, 0), (5, 0, 0), (6, n - 1, 2)):
        assert dev.debug_verify_plant(part, e, off) == 0
        res = call(-5)
        bad += 1
        assert res.error == head + f'first episode {e} ({PART_NAMES[part]}{"" if part >= 2 else " "}); no recorded trajectory row differs', (part, res.error)
        assert dev.verify_stats() == (1 + bad + (bad > 1), bad)          # (one clean call in front, one more behind the first reported one)
        if bad == 1:
            call()
            assert dev.verify_stats() == (3, 1)
    # the recorded trajectory: first, a middle and the last step; first, a middle and the last episode
    for part in (7, 8, 9):
        for step, e in ((0, n - 1), (K // 2, 0), (K - 1, mid)):
            off = (0, H.OBS_PACKED - 1, 70)[step % 3] if part == 9 else 0
            assert dev.debug_verify_plant(part, e, off, step) == 0
            res = call(-5)
            bad += 1
            assert res.error == head + f'first differing trajectory row: {TRAJ_NAMES[part]} of step {step}, 1 episode(s) differ in it, first episode {e}', (part, step, res.error)
            assert _parse(res.error) is None
    checked, disagreed = dev.verify_stats()
    assert (checked, disagreed) == (2 + bad, bad) and bad == 16
    # a trajectory part the call cannot apply: nothing is stepped, nothing stays armed
    rows = dev.get_states()
    assert dev.debug_verify_plant(7, 0, 0, K) == 0           # step K of a K-step plan
    call(-2)
    assert dev.verify_stats() == (checked, disagreed) and np.array_equal(dev.get_states(), rows)
    call()
    assert dev.verify_stats() == (checked + 1, disagreed)
    _same_as_oracle(dev, ora, state['out'], state['act'], kernel)
    dev.close(), ora.close()


# ------------------------------------------------------------------------------------------------ the sampled default
def test_the_sampled_check_reports_a_plant_at_the_call_it_checks(monkeypatch):
    from cage_challenge_4_amd._lib import CC4Error
    _clean_env(monkeypatch, CC4_PERSIST_VERIFY_EVERY='2')
    n = N_PHILOX1
    dev = _dev(n, rng_mode=1)
    dev.reset(seeds=5)
    assert dev.run_kernel_for(K) == 'k_run_philox1'
    assert dev.debug_verify_plant(1, n - 1, 5) == 0
    dev.run_random_steps(5, 0, K, timed=False)               # call 1: not checked, the plant survives it
    assert dev.verify_stats() == (0, 0)
    with pytest.raises(CC4Error) as ei:                      # call 2: checked
        dev.run_random_steps(5, K, K, timed=False)
    assert 'rc=-5' in str(ei.value) and _parse(str(ei.value)) == (n - 1, ['cold row']), str(ei.value)
    assert dev.verify_stats() == (1, 1)
    dev.run_random_steps(5, 2 * K, K, timed=False)
    dev.run_random_steps(5, 3 * K, K, timed=False)           # call 4: checked, clean
    assert dev.verify_stats() == (2, 1) and not dev.err.any()
    dev.close()


def test_a_handle_that_never_checks_refuses_the_hook(monkeypatch):
    _clean_env(monkeypatch, CC4_PERSIST_VERIFY_EVERY='0')
    dev = _dev(N_PHILOX1, rng_mode=1)
    dev.reset(seeds=5)
    assert dev.run_kernel_for(K) == 'k_run_philox1'
    assert dev.debug_verify_plant(0, 0, 0) == -2 and 'ever checked' in dev.lib.cc4_last_error(dev._h).decode()
    for t in range(3):
        dev.run_random_steps(5, t * K, K, timed=False)
    assert dev.verify_stats() == (0, 0) and H.shadow_handle(dev) is None
    dev.close()


# ------------------------------------------------------------------------------------------------ refusals
def test_refusals_leave_nothing_armed(monkeypatch):
    from cage_challenge_4_amd._lib import CC4Error
    _clean_env(monkeypatch, CC4_PERSIST_VERIFY='1')
    n = 64
    dev = _dev(n, rng_mode=1)
    dev.reset(seeds=6)
    assert dev.run_kernel_for(K) == 'k_run_philox'
    hot, cold = int(dev.lib.cc4_state_bytes()), int(dev.lib.cc4_cold_bytes(dev._h))
    t = 0
    for part, e, off, step in ((10, 0, 0, 0), (-2, 0, 0, 0), (0, n, 0, 0), (0, -1, 0, 0), (0, 0, hot, 0), (0, 0, -1, 0), (1, 0, cold, 0), (2, 0, D.OBS, 0),
                               (3, 0, 1, 0), (4, 0, 1, 0), (5, 0, 1, 0), (6, 0, D.NBLUE, 0), (0, 0, 0, 1), (7, 0, 1, 0), (8, 0, 0, -1), (9, 0, H.OBS_PACKED, 0)):
        assert dev.debug_verify_plant(0, 1, 2) == 0          # something armed: a refused call of the hook takes it away
        assert dev.debug_verify_plant(part, e, off, step) == -2, (part, e, off, step)
        dev.run_random_steps(6, t, K, timed=False)           # a checked call, clean
        t += K
    checked = dev.verify_stats()
    assert checked == (16, 0)
    assert dev.debug_verify_plant(0, 1, 2) == 0 and dev.debug_verify_plant(-1) == 0       # disarmed by hand
    dev.run_random_steps(6, t, K, timed=False)
    t += K
    # a trajectory part meets a call that records no trajectory: refused there, nothing stepped, nothing armed
    rows = dev.get_states()
    assert dev.debug_verify_plant(8, 3, 0, 2) == 0
    with pytest.raises(CC4Error) as ei:
        dev.run_random_steps(6, t, K, timed=False)
    assert 'rc=-2' in str(ei.value) and 'cc4_debug_verify_plant' in str(ei.value)
    assert dev.verify_stats() == (17, 0) and np.array_equal(dev.get_states(), rows)
    dev.run_random_steps(6, t, K, timed=False)
    assert dev.verify_stats() == (18, 0)
    # the shadow handle itself
    sh = H.shadow_handle(dev)
    assert sh is not None and dev.lib.cc4_debug_verify_plant(sh, 0, 0, 0, 0) == -2
    dev.close()


def test_a_handle_with_a_communicator_refuses_the_hook(monkeypatch):
    _clean_env(monkeypatch, CC4_PERSIST_VERIFY='1')
    one = _dev(4, rng_mode=1)
    one.reset(seeds=5)
    os.environ.setdefault('NCCL_SOCKET_IFNAME', 'lo')
    ident = (ctypes.c_uint8 * 128)()
    assert one.lib.cc4_comm_unique_id(ident) == 0
    one._chk(one.lib.cc4_comm_init(one._h, 0, 1, ident), 'cc4_comm_init')
    assert one.debug_verify_plant(0, 0, 0) == -2 and 'communicator' in one.lib.cc4_last_error(one._h).decode()
    one.close()
