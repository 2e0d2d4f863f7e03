"""GPU: every kernel against the oracle on episodes whose bounded containers are one below, at and past their capacity (tests/capacity_util.py
crafts them on the oracle; tests/test_capacity_cpu.py shows that the 'over' variants raise their flags there while their 'cap' twins stay clean,
which is what keeps the comparisons here from passing vacuously).  The crafted episodes are moved into the device batch with
dev.restore(e, ora.snapshot(e)); every step's observations, rewards, dones and err words are compared, and at the end the hot and cold rows of
the crafted episodes and of the episode behind each one -- a store past a capacity lands in the neighbouring field or in the next episode's row.

* the three step kernels in small batches: the operation's edits (the same return value on both sides), then a first step with the submitted
  exploits / phishing e-mails / DeployDecoy / Monitor actions of the scenarios, then seeded random blue actions;
* the persistent kernels (k_run_philox1 at 6656 episodes, k_run_pcg at 5000, autoreset on) with a crafted variant on every eighth episode, calls
  of 10, 3, 25 and 1 steps, and one plan of 12 steps on the counter-mode handle;
* once: clone, save and load of the at-capacity episodes (hot row and the live extents of the cold row equal the source's, the episodes behind
  the destinations untouched) and the state features of the full-pool episodes."""
import ctypes

import numpy as np
import pytest

import capacity_util as U
from oracle_binding import OracleVecEnv, random_actions

pytestmark = pytest.mark.gpu
SEED = 1030                      # tests/test_capacity_cpu.py: with episode seed SEED + scenario index every first step does what its operation says
KERNELS = {'4wave': (65, 1, '0', 'k_step_philox'), '1wave': (40, 1, '1', 'k_step_philox1'), 'numpy_stream': (33, 0, None, 'k_step')}


def _dev(n, **kw):
    from cage_challenge_4_amd import CC4VecEnv
    return CC4VecEnv(n, strict=False, **kw)


def _chunks():
    out = []
    for kid, (n, _m, _l, _k) in KERNELS.items():
        per = (n - 1) // 2                           # crafted on the even episodes, each with an untouched episode behind it
        for c0 in range(0, len(U.SCENARIOS), per):
            out.append(pytest.param(kid, c0, per, id=f'{kid}-{c0}'))
    return out


def _bad(d, o):
    return np.nonzero((d[0] != o[0]).any(axis=1) | (d[1] != o[1]) | (np.asarray(d[2], bool) != np.asarray(o[2], bool)) | (d[3]['err'] != o[3]['err']))[0]


def _rows_equal(dev, ora, episodes, what):
    for e in episodes:
        (h1, c1), (h2, c2) = dev.snapshot(e), ora.snapshot(e)
        assert np.array_equal(h1, h2), (what, e, 'hot row', np.nonzero(h1 != h2)[0][:20].tolist())
        assert np.array_equal(c1, c2), (what, e, 'cold row', np.nonzero(c1 != c2)[0][:20].tolist())


@pytest.mark.parametrize('kid,c0,per', _chunks())
def test_step_kernel_matches_oracle_at_and_past_capacity(monkeypatch, kid, c0, per):
    n, mode, lean, kernel = KERNELS[kid]
    if lean is not None:
        monkeypatch.setenv('CC4_PHILOX_LEAN', lean)
    cp = U.caps()
    names = U.SCENARIOS[c0:c0 + per]
    dev = _dev(n, steps=U.STEPS, rng_mode=mode)
    assert dev.step_kernel == kernel
    ora = OracleVecEnv(n, steps=U.STEPS, rng_mode=mode)
    seeds = np.arange(n, dtype=np.uint64) + np.uint64(7000)
    for i in range(len(names)):
        seeds[2 * i] = SEED + c0 + i
    assert np.array_equal(dev.reset(seeds=seeds), ora.reset(seeds=seeds))
    built = {}
    for i, sc in enumerate(names):
        built[2 * i] = U.build(ora, 2 * i, sc)
        dev.restore(2 * i, ora.snapshot(2 * i))
    for e, b in built.items():                       # the operation's edits: the same value from the library and from the oracle
        got, want = U.apply_edits(dev, e, b), U.apply_edits(ora, e, b)
        assert got == want == [x[4] for x in b.edits], (b.scenario, got, want)
    (red, green), blue = U.submissions(ora, built)
    T = 24
    for t in range(T):
        acts = random_actions(SEED, t, n)
        if t == 0:
            acts = U.first_step_actions(acts, blue)
            d = dev.step_ex(acts, None, red, green); o = ora.step_ex(acts, None, red, green)
            for e, b in built.items():               # not vacuous: the flag is there on both sides, the twins are clean
                assert int(o[3]['err'][e]) == b.expect and int(d[3]['err'][e]) == b.expect, (b.scenario, int(d[3]['err'][e]), int(o[3]['err'][e]), b.expect)
        elif t % 3 == 1:
            d = dev.step(acts); o = ora.step(acts)
        else:
            d = dev.step_ex(acts, None, None, None); o = ora.step_ex(acts, None, None, None)
        bad = _bad(d, o)
        assert bad.size == 0, (t, [(int(e), built[e].scenario if e in built else 'neighbour') for e in bad[:8]])
    assert {cp[f] for f in ('E_PROC', 'E_RSESS', 'E_KS', 'E_SUS', 'E_PEND')} >= {b.expect for b in built.values()} - {0}
    _rows_equal(dev, ora, sorted(set(built) | {e + 1 for e in built}), kid)
    dev.close(); ora.close()


def _craft_every_eighth(dev, ora, n):
    built = {}
    for k, e in enumerate(range(0, n - 1, 8)):
        built[e] = U.build(ora, e, U.SCENARIOS[k % len(U.SCENARIOS)])
        dev.restore(e, ora.snapshot(e))
    for e, b in built.items():
        got, want = U.apply_edits(dev, e, b), U.apply_edits(ora, e, b)
        assert got == want == [x[4] for x in b.edits], (b.scenario, got, want)
    return built


@pytest.mark.parametrize('n,mode,kernel', [(6656, 1, 'k_run_philox1'), (5000, 0, 'k_run_pcg')], ids=['k_run_philox1', 'k_run_pcg'])
def test_persistent_kernel_matches_oracle_at_and_past_capacity(n, mode, kernel):
    """No submitted actions here (the kernels draw the blue actions themselves): the operations that are edits or part of the crafted state --
    the refused 65th session and decoy, the reassignment into a full agent, the known-id list, the pending events -- raise their flags on the
    first step, the rest is whatever 39 steps of play make of full containers, on both sides alike."""
    cp = U.caps()
    seed0 = 4040
    dev = _dev(n, steps=U.STEPS, rng_mode=mode, autoreset=True)
    assert dev.run_kernel_for(10) == kernel and dev.run_kernel_for(3) != kernel
    ora = OracleVecEnv(n, steps=U.STEPS, rng_mode=mode, autoreset=True)
    assert np.array_equal(dev.reset(seeds=seed0), ora.reset_batch(seed0))
    built = _craft_every_eighth(dev, ora, n)
    seen = np.zeros(n, np.uint32)
    t = 0
    for K in (10, 3, 25, 1):
        dev.run_random_steps(seed0, t, K, timed=False)
        for k in range(K):
            o = ora.step_batch(random_actions(seed0, t + k, n))
            seen |= o[3]['err']
        t += K
        dev.synchronize(); dev._fetch()
        bad = np.nonzero((dev._obs != o[0]).any(axis=1) | (dev._rew != o[1]) | (dev._done.astype(bool) != o[2]) | (dev._err != o[3]['err']))[0]
        assert bad.size == 0, (K, t, [(int(e), built[e].scenario if e in built else 'plain') for e in bad[:8]])
    if mode == 1:                                    # one plan of 12 steps on the counter-mode handle
        K = 12
        plan = np.stack([random_actions(seed0 + 1, t + k, n) for k in range(K)])
        obs, rew, done, info = dev.run_plan(plan)
        raised = np.zeros(n, np.uint32)
        for k in range(K):
            o = ora.step_batch(plan[k])
            raised |= o[3]['err']
            assert np.array_equal(rew[k], o[1]) and np.array_equal(done[k], o[2]), (k, np.nonzero(rew[k] != o[1])[0][:8].tolist())
        seen |= raised
        # (the handle's err words after a plan: at least the last step's, at most what the plan's steps showed)
        assert np.array_equal(obs, o[0]) and not (o[3]['err'] & ~info['err']).any() and not (info['err'] & ~raised).any()
    # not vacuous: the flags whose operation needs no submitted action came up in crafted episodes, their twins' first call stayed clean on both sides
    crafted_flags = 0
    for e in built:
        crafted_flags |= int(seen[e])
    for f in ('E_PROC', 'E_RSESS', 'E_KS', 'E_SUS'):
        assert crafted_flags & cp[f], (f, crafted_flags)
    rows = dev.get_states()
    bad = [e for e in range(n) if not np.array_equal(rows[e], ora.get_state(e))]
    assert not bad, [(e, built[e].scenario if e in built else 'plain') for e in bad[:8]]
    for e in sorted(set(list(built)[::7]) | {e + 1 for e in list(built)[::7]} | {n - 1}):       # cold rows: a sample of the crafted episodes and their neighbours
        c1, c2 = dev.get_cold(e), ora.get_cold(e)
        assert np.array_equal(c1, c2), (e, 'cold row', np.nonzero(c1 != c2)[0][:20].tolist())
    dev.close(); ora.close()


def test_copies_and_features_of_full_containers():
    """clone / save / load of every at-capacity episode: the destination's hot row and the live extents of its cold row are the source's -- to the
    last entry of a full list --, the episodes behind the destinations are untouched; k_state_features strides over a full pool."""
    from cage_challenge_4_amd import state_features as SF
    from view_util import DevMem
    mode = 1
    caps_ = [sc for sc in U.SCENARIOS if sc.endswith(':cap')] + ['proc_pin:over', 'proc_pin:m1']
    m = len(caps_)
    n = 4 * m + 2            # sources 0 .. m-1, clone destinations m + 2i, load destinations 3m + 1 .. 4m (behind them: episode 4m + 1)
    dev = _dev(n, steps=U.STEPS, rng_mode=mode)
    ora = OracleVecEnv(n, steps=U.STEPS, rng_mode=mode)
    seeds = np.arange(n, dtype=np.uint64) + np.uint64(SEED)
    assert np.array_equal(dev.reset(seeds=seeds), ora.reset(seeds=seeds))
    for e, sc in enumerate(caps_):
        U.build(ora, e, sc)
        dev.restore(e, ora.snapshot(e))
    for t in range(2):                                   # two steps, so that the destinations' own rows hold something else than zeros
        d = dev.step(random_actions(SEED, t, n)); o = ora.step(random_actions(SEED, t, n))
        assert _bad(d, o).size == 0
    before = {e: dev.snapshot(e) for e in range(n)}
    live = lambda snap: U.live_cold(snap[0], snap[1], U.STEPS, mode)                        # noqa: E731
    src = np.arange(m, dtype=np.int32)
    dst = (m + 2 * np.arange(m)).astype(np.int32)
    dev.clone_episodes(src, dst)
    for s, d_ in zip(src, dst):
        got = dev.snapshot(int(d_))
        assert np.array_equal(got[0], before[int(s)][0]) and live(got) == live(before[int(s)]), (caps_[s], 'clone')
        nb = dev.snapshot(int(d_) + 1)
        assert np.array_equal(nb[0], before[int(d_) + 1][0]) and np.array_equal(nb[1], before[int(d_) + 1][1]), (caps_[s], 'behind the clone')
    # save into a bank, load into the last m episodes
    slot = int(dev.lib.cc4_snapshot_bytes(dev._h))
    bank, idx = DevMem(m * slot), DevMem(4 * 3 * m + 64)
    slots = np.arange(m, dtype=np.int32)[::-1].copy()
    ld = (3 * m + 1 + np.arange(m)).astype(np.int32)
    off_b, off_c = (4 * m + 15) & ~15, 2 * ((4 * m + 15) & ~15)
    idx.up(src); idx.up(slots, off_b); idx.up(ld, off_c)
    lib, h = dev.lib, dev._h
    assert lib.cc4_copy_episodes_device(h, m, None, 0, idx.p, bank.p, m, idx.at(off_b), None) == 0, lib.cc4_last_error(h)
    assert lib.cc4_copy_episodes_device(h, m, bank.p, m, idx.at(off_b), None, 0, idx.at(off_c), None) == 0, lib.cc4_last_error(h)
    f = ctypes.c_uint32(0)
    assert lib.cc4_copy_faults(h, ctypes.byref(f)) == 0 and f.value == 0
    for s, d_ in zip(src, ld):
        got = dev.snapshot(int(d_))
        assert np.array_equal(got[0], before[int(s)][0]) and live(got) == live(before[int(s)]), (caps_[s], 'load')
    last = dev.snapshot(n - 1)
    assert np.array_equal(last[0], before[n - 1][0]) and np.array_equal(last[1], before[n - 1][1])
    for e in range(m, 3 * m + 1):                        # everything between the clones' region and the loads': as the clones left it
        if e not in set(dst.tolist()):
            now = dev.snapshot(e)
            assert np.array_equal(now[0], before[e][0]) and np.array_equal(now[1], before[e][1]), e
    # a copy behaves as its source: a step of all of them
    acts = random_actions(SEED, 2, n)
    acts[dst] = acts[src]; acts[ld] = acts[src]
    obs, rew, done, info = dev.step(acts)
    assert np.array_equal(obs[dst], obs[src]) and np.array_equal(obs[ld], obs[src]) and np.array_equal(info['err'][dst], info['err'][src]) and np.array_equal(rew[ld], rew[src])
    # the features of the full-pool episodes (and of every other one) against the host statement of the same definition
    hosts, glob = dev.state_features()
    rows = dev.get_states()
    full_pool = [e for e, sc in enumerate(caps_) if sc.startswith('pool')]
    assert len(full_pool) == 5 and all(int(glob[e, 17:23].sum()) >= U.caps()['RS_POOL'] - 24 for e in full_pool)
    for e in range(n):
        wh, wg = SF.from_row(rows[e])
        assert np.array_equal(hosts[e], wh) and np.array_equal(glob[e], wg), e
    bank.free(); idx.free()
    dev.close(); ora.close()
