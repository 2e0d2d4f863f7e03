"""GPU: the red agents' header and the action records held as words (csrc/cc4_state.h: RedHdrW / ActW; the policy / tick path, the blue queue,
the head of the red and blue actions) against the CPU oracle.  tests/test_hdr_words_cpu.py checks the accessors against member access; here the
kernels that carry them play, and after EVERY step the observations, rewards, dones, error words, generator states and the whole hot rows of
all episodes must be the oracle's:

* the per-step kernels -- k_step_philox1 in its fast and its full build, k_step_philox, k_step -- on 256 episodes of 40 steps stepped 60
  times with autoreset, so that every episode ends and regenerates once on the way (the header a regeneration writes is the one the next
  tick loads);
* the same kernels on 64 episodes of 1000 steps stepped 300 times: fsm_step, a 16-bit field in the upper half of its word, passes 255 (the
  count on the word carries into the field's second byte).  new_sess_id, in the word next to it, is no count: it is the id of the session the
  agent's Exploit made on this step, and 300 steps of play hand out ids up to the low twenties (printed) -- it passes 255 in the next case;
* the per-step kernels from the crafted states of tests/capacity_util.py with a 64-entry session list (nsess = MAX_RS, the byte next to
  nknown), the known-id count at MAX_KS - 1 and at MAX_KS, and an agent one of whose sessions carries id 300, so that the session its Exploit
  makes on the first step is number 301: new_sess_id == 301 is asserted on both sides after that step and after the next tick;
* the persistent kernels k_run_philox1 and k_run_philox1p at 6656 episodes of 40 steps (the smallest batch they take), calls of 12 and 45 steps
  under the library's self-check, compared after each call.

The oracle's side of each (mode, shape) is computed once and shared by the kernels of that mode."""
import ctypes
import hashlib

import numpy as np
import pytest

import capacity_util as U
from oracle_binding import OracleVecEnv, random_actions

pytestmark = pytest.mark.gpu

# kernel id -> (rng_mode, CC4_PHILOX_LEAN, the full build (cc4_step_ex) instead of the fast one, cc4_step_kernel)
KERNELS = {'k_step_philox1-fast': (1, '1', False, 'k_step_philox1'), 'k_step_philox1-full': (1, '1', True, 'k_step_philox1'),
           'k_step_philox': (1, '0', False, 'k_step_philox'), 'k_step': (0, None, False, 'k_step')}
_REF = {}


def _dev(n, **kw):
    from cage_challenge_4_amd import CC4VecEnv
    return CC4VecEnv(n, strict=False, **kw)


def _digest(rows):
    return [hashlib.blake2b(np.ascontiguousarray(r).tobytes(), digest_size=16).digest() for r in rows]


def _ora_step(ora, acts, full):
    """ora.step, or its twin through cc4o_step_ex with no action submitted (what the device's full build is handed), autoreset included."""
    if not full:
        return ora.step(acts)
    from cage_challenge_4_amd._lib import AGENT_ACTION_DTYPE
    lib = ora.lib
    lib.cc4o_step_ex.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]
    ext = np.zeros(86, dtype=AGENT_ACTION_DTYPE)
    ext['type'] = -1
    for i in range(ora.num_envs):
        if ora.autoreset and ora._done[i]:
            lib.cc4o_reset(ora._h, i, 0, ora.rng_mode, ora.steps, 1, ora.policy)
            ora._collect(i, reward=False)
            continue
        a = np.ascontiguousarray(acts[i], np.int32)
        lib.cc4o_step_ex(ora._h, i, a.ctypes.data_as(ctypes.c_void_p), None, ext.ctypes.data_as(ctypes.c_void_p))
        ora._collect(i)
    return ora._obs, ora._rew, ora._done, {'err': ora._err}


def _record(ora, o):
    return (o[0].copy(), o[1].copy(), np.asarray(o[2], bool).copy(), o[3]['err'].copy(), ora.rng_state(),
            _digest(ora.get_state(e) for e in range(ora.num_envs)))


def _reference(mode, full, n, steps, T, seed):
    """The oracle's trajectory of T steps of seeded random blue actions: per step (obs, reward, done, err, generator states, row digests), the first
    observation, how often each episode regenerated, and the largest fsm_step and new_sess_id seen (every eighth episode)."""
    key = (mode, full, n, steps, T, seed)
    if key not in _REF:
        ora = OracleVecEnv(n, steps=steps, rng_mode=mode, autoreset=True)
        first = ora.reset(seeds=seed).copy()
        traj, regen = [], np.zeros(n, int)
        L = U.layout()
        peak = {'fsm_step': 0, 'new_sess_id': 0}
        for t in range(T):
            regen += ora._done
            traj.append(_record(ora, _ora_step(ora, random_actions(seed, t, n), full)))
            for e in range(0, n, 8):
                row = ora.get_state(e)
                for r in range(6):
                    for f in peak:
                        off = L['red'] + r * L['sizeof.RedAgent'] + L['red.' + f]
                        peak[f] = max(peak[f], int(row[off]) | int(row[off + 1]) << 8)
        ora.close()
        _REF[key] = (first, traj, regen, peak)
    return _REF[key]


def _compare(dev, d, want, t, what):
    obs, rew, done, err, rng, digests = want
    bad = np.nonzero((d[0] != obs).any(axis=1) | (d[1] != rew) | (np.asarray(d[2], bool) != done) | (d[3]['err'] != err))[0]
    assert bad.size == 0, (what, t, 'outputs', bad[:10].tolist())
    got = dev.rng_state()
    bad = np.nonzero((got != rng).any(axis=1))[0]
    assert bad.size == 0, (what, t, 'generator state', bad[:10].tolist())
    got = _digest(dev.get_states())
    bad = [e for e in range(dev.num_envs) if got[e] != digests[e]]
    assert not bad, (what, t, 'hot row', bad[:10])


def _play(monkeypatch, kid, n, steps, T, seed):
    mode, lean, full, kernel = KERNELS[kid]
    if lean is not None:
        monkeypatch.setenv('CC4_PHILOX_LEAN', lean)
    first, traj, regen, peak = _reference(mode, full, n, steps, T, seed)
    dev = _dev(n, steps=steps, rng_mode=mode, autoreset=True)
    assert dev.step_kernel == kernel
    assert np.array_equal(dev.reset(seeds=seed), first)
    for t in range(T):
        acts = random_actions(seed, t, n)
        d = dev.step_ex(acts, None, None, None) if full else dev.step(acts)
        _compare(dev, d, traj[t], t, kid)
    dev.close()
    return regen, peak


@pytest.mark.parametrize('kid', list(KERNELS))
def test_every_step_through_a_regeneration(monkeypatch, kid):
    regen, _ = _play(monkeypatch, kid, 256, 40, 60, 9100)
    assert (regen == 1).all(), regen[:16].tolist()            # every episode ended and regenerated once


@pytest.mark.parametrize('kid', list(KERNELS))
def test_every_step_while_the_counters_pass_255(monkeypatch, kid):
    _, peak = _play(monkeypatch, kid, 64, 1000, 300, 9200)
    print('largest values reached:', peak)
    assert peak['fsm_step'] > 256, peak                        # the count crossed the byte boundary inside its field


@pytest.mark.parametrize('kid', list(KERNELS))
def test_full_session_list_and_known_ids_at_capacity(monkeypatch, kid):
    """Crafted episodes (tests/capacity_util.py) on the even episodes, an untouched one behind each: a 64-entry session list made by an edit, by an
    Exploit and by the reassignment, and the known-id list at MAX_KS - 1 (the step's new session fills it) and at MAX_KS, with ids below and
    past 255.  The first step carries the scenarios' submitted actions (cc4_step_ex); then the kernel's own build, 24 steps in all."""
    mode, lean, full, kernel = KERNELS[kid]
    if lean is not None:
        monkeypatch.setenv('CC4_PHILOX_LEAN', lean)
    names = ['rs_add:m1', 'rs_add:cap', 'rs_exploit:m1', 'rs_exploit:cap', 'rs_reassign:m1', 'rs_reassign:cap', 'known:m1', 'known:cap', 'known256:m1', 'known256:cap',
             'rs_exploit:m1']        # (the last one: with a session id of 300 in the agent's list, below)
    E_ID = 2 * (len(names) - 1)
    n = 2 * len(names) + 1
    cp = U.caps()
    dev = _dev(n, steps=U.STEPS, rng_mode=mode)
    assert dev.step_kernel == kernel
    ora = OracleVecEnv(n, steps=U.STEPS, rng_mode=mode)
    seeds = np.arange(n, dtype=np.uint64) + np.uint64(7000)
    for i, sc in enumerate(names):
        seeds[2 * i] = 1030 + U.SCENARIOS.index(sc)          # tests/test_capacity_cpu.py: with this seed the scenario's first step does what its operation says
    assert np.array_equal(dev.reset(seeds=seeds), ora.reset(seeds=seeds))
    built = {}
    L = U.layout()
    sid_off = L['red'] + 1 * L['sizeof.RedAgent'] + L['red.new_sess_id']
    for i, sc in enumerate(names):
        built[2 * i] = U.build(ora, 2 * i, sc)
        if 2 * i == E_ID:
            # the second session of red_agent_1's list (not the primary, not the one the Exploit starts from) gets id 300: State.add_session hands out
            # max + 1, so the session this step's Exploit makes is number 301 and new_sess_id holds a value past 255
            hot, cold = ora.snapshot(E_ID)
            slot = int(hot[L['red'] + 1 * L['sizeof.RedAgent'] + L['red.sord'] + 1])
            off = L['spool'] + slot * L['sizeof.RSess'] + L['rsess.id']
            assert 0 < (int(hot[off]) | int(hot[off + 1]) << 8) < 255 and built[E_ID].red[0][3] != (int(hot[off]) | int(hot[off + 1]) << 8)
            hot[off], hot[off + 1] = 300 & 0xFF, 300 >> 8
            ora.restore(E_ID, (hot, cold))
        dev.restore(2 * i, ora.snapshot(2 * i))
    for e, b in built.items():
        got, want = U.apply_edits(dev, e, b), U.apply_edits(ora, e, b)
        assert got == want == [x[4] for x in b.edits], (b.scenario, got, want)
    (red, green), blue = U.submissions(ora, built)
    full_lists = full_known = 0
    T = 24
    for t in range(T):
        acts = random_actions(1030, t, n)
        if t == 0:
            acts = U.first_step_actions(acts, blue)
            d = dev.step_ex(acts, None, red, green); o = ora.step_ex(acts, None, red, green)
        elif full or t == T - 1:     # (the last step through cc4_step_ex for every kernel: EnvCold.gfail, which the cold rows are compared with below, is the full builds')
            d = dev.step_ex(acts, None, None, None); o = ora.step_ex(acts, None, None, None)
        else:
            d = dev.step(acts); o = ora.step(acts)
        _compare(dev, d, _record(ora, o), t, kid)
        if t <= 1:       # the Exploit's session is number 301: in the header after the step that made it, and still after the next tick loaded and stored the word
            for row in (ora.get_state(E_ID), dev.get_state(E_ID)):
                assert (int(row[sid_off]) | int(row[sid_off + 1]) << 8) == 301, (t, int(row[sid_off]) | int(row[sid_off + 1]) << 8)
        if t == 0:
            for e, b in built.items():                                           # 'm1' ends exactly full, 'cap' stays full: the first step overflows nothing
                assert int(o[3]['err'][e]) == 0 and int(d[3]['err'][e]) == 0, (b.scenario, int(d[3]['err'][e]), int(o[3]['err'][e]))
            for e in built:
                row = ora.get_state(e)
                for r in range(6):
                    base = L['red'] + r * L['sizeof.RedAgent']
                    full_lists += int(row[base + L['red.nsess']]) == cp['MAX_RS']
                    full_known += int(row[base + L['red.nknown']]) == cp['MAX_KS']
    assert full_lists >= 4 and full_known >= 3, (full_lists, full_known)         # not vacuous: the lists were full when the next tick loaded the header
    for e in sorted(set(built) | {e + 1 for e in built}):
        c1, c2 = dev.get_cold(e), ora.get_cold(e)
        assert np.array_equal(c1, c2), (kid, e, 'cold row', np.nonzero(c1 != c2)[0][:20].tolist())
    dev.close(); ora.close()


def _persistent_reference(n, steps, calls, seed):
    key = ('persistent', n, steps, calls, seed)
    if key not in _REF:
        ora = OracleVecEnv(n, steps=steps, rng_mode=1, autoreset=True)
        ora.reset_batch(seed)
        out, t = [], 0
        for K in calls:
            for k in range(K):
                o = ora.step_batch(random_actions(seed, t + k, n))
            t += K
            out.append(_record(ora, o))
        ora.close()
        _REF[key] = out
    return _REF[key]


@pytest.mark.parametrize('kernel', ['k_run_philox1', 'k_run_philox1p'])
def test_persistent_kernels_under_the_self_check(monkeypatch, kernel):
    """Calls of 12 and 45 steps at 6656 episodes of 40 steps (every episode regenerates inside the second call).  k_run_philox1 draws the stand-in
    policy's blue actions in the kernel, k_run_philox1p reads the same actions from a plan on the device: one reference for both."""
    monkeypatch.delenv('CC4_PERSIST_MIN_K', raising=False)
    monkeypatch.delenv('CC4_PHILOX_LEAN', raising=False)
    monkeypatch.setenv('CC4_PERSIST_VERIFY', '1')
    n, steps, calls, seed = 6656, 40, (12, 45), 9300
    want = _persistent_reference(n, steps, calls, seed)
    dev = _dev(n, steps=steps, rng_mode=1, autoreset=True)
    dev.reset(seeds=seed)
    t = 0
    for i, K in enumerate(calls):
        if kernel == 'k_run_philox1':
            assert dev.run_kernel_for(K) == kernel
            dev.run_random_steps(seed, t, K, timed=False)
        else:
            assert dev.plan_kernel_for(K) == kernel
            dev.run_plan(np.stack([random_actions(seed, t + k, n) for k in range(K)]))
        t += K
        dev.synchronize(); dev._fetch()
        _compare(dev, (dev._obs, dev._rew, dev._done, {'err': dev._err}), want[i], t, kernel)
        assert dev.verify_stats() == (i + 1, 0)
    dev.close()
