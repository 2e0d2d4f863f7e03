"""GPU: the reward terms from the device.  cc4_reward_terms_device (k_reward_terms) on each of the three step kernels against the host statement of
the same definition (reward_terms.from_row) on the device's own rows and on the oracle's rows, with the first identity against the fetched
reward, through regenerations; id lists, an id out of range, snapshot banks read in place, clone_episodes carrying the record, the switch off
and the event log alone; and the cells of the reference's BlueRewardMachine fixtures on the numpy-stream kernel."""
import ctypes

import numpy as np
import pytest

from cage_challenge_4_amd import reward_terms as RT
from oracle_binding import OracleVecEnv
import reward_terms_util as U
import test_scripted as TS
from view_util import DevMem, _dev, _faults, call_view

pytestmark = pytest.mark.gpu

ROW_T, ROW_W = 9 * 4 * 4, 16 * 4
CF_RANGE, CF_SLOT_EMPTY = 1, 8
KERNELS = [('k_step', 0, None), ('k_step_philox', 1, '0'), ('k_step_philox1', 1, '1')]


def _make(kernel, mode, lean, monkeypatch, n, **kw):
    if lean is not None:
        monkeypatch.setenv('CC4_PHILOX_LEAN', lean)
    dev = _dev(n, rng_mode=mode, **kw)
    assert dev.step_kernel == kernel
    return dev


def _view(dev, n, ids=None, bank=None, cap=0, fill=0, words=True):
    """cc4_reward_terms_device into a fresh device buffer [terms | words], then synchronise and copy down."""
    def call(d_bank, cap, d_ids, n, p_terms, p_words):
        dev.reward_terms_device(p_terms, p_words, n=n, d_ids=d_ids, d_bank=d_bank, capacity=cap)
    return call_view(dev, call, n, ((np.int32, (9, 4)), (np.int32, (16,))), ids, bank, cap, fill, second=words)


@pytest.mark.parametrize('kernel,mode,lean', KERNELS, ids=[k[0] for k in KERNELS])
def test_kernel_host_function_and_oracle_agree_through_regenerations(kernel, mode, lean, monkeypatch):
    n, steps, T, seed = 70, 12, 40, 8100
    dev = _make(kernel, mode, lean, monkeypatch, n, steps=steps, autoreset=True, strict=False)
    ora = OracleVecEnv(n, steps=steps, rng_mode=mode, autoreset=True)
    assert np.array_equal(dev.reset(seeds=seed), ora.reset(seeds=seed))
    assert not dev.reward_terms_enabled
    dev.enable_reward_terms()
    assert dev.reward_terms_enabled and dev.run_kernel_for(20) == kernel            # one launch per step from here on
    terms, words = dev.reward_terms()
    assert terms.shape == (n, 9, 4) and terms.dtype == np.int32 and words.shape == (n, 16) and words.dtype == np.int32
    assert not terms.any() and not words.any(), 'fresh episodes'
    seen = dict(valid=0, stale=0, lwf=0, asf=0, ria=0, restore=0, zero_weight=0)
    for t in range(T):
        acts = U.blue_mix(seed, t, n)
        acts[t % n, 3] = U.restore_code(ora, t % n, 3)                               # (the mix's own Restores are few in 12-step episodes)
        d = dev.step(acts)
        o = U.oracle_step_recording(ora, acts)
        assert np.array_equal(d[0], o[0]) and np.array_equal(d[1], o[1]) and np.array_equal(d[2], o[2]) and not d[3]['err'].any(), t
        terms, words = dev.reward_terms()
        ht, hw = U.from_rows(dev, range(n), steps)
        ot, ow = U.from_rows(ora, range(n), steps)
        assert np.array_equal(terms, ht) and np.array_equal(words, hw), (t, np.argwhere(terms != ht)[:6].tolist(), np.argwhere(words != hw)[:6].tolist())
        assert np.array_equal(terms, ot) and np.array_equal(words, ow), (t, np.argwhere(terms != ot)[:6].tolist(), np.argwhere(words != ow)[:6].tolist())
        U.check_identities(terms, words, d[1], (kernel, t))
        v = words[:, 0] == 1
        regenerated = words[:, 1] == 0
        assert np.array_equal(v, ~regenerated), t                                    # every step recorded; a regenerated episode has taken none
        seen['valid'] += int(v.sum()); seen['stale'] += int((~v).sum())
        seen['lwf'] += int((terms[..., 0] != 0).any(1).sum()); seen['asf'] += int((terms[..., 1] != 0).any(1).sum())
        seen['ria'] += int((terms[..., 2] != 0).any(1).sum()); seen['restore'] += int((words[:, 4] != 0).sum())
        seen['zero_weight'] += int((terms[..., 3] > 0)[terms[..., :3].sum(2) == 0].sum())
    # not vacuous (LocalWork rarely fails in the first twelve steps of an episode: test_long_episodes_on_the_device has its share)
    assert seen['stale'] >= 2 * n and seen['lwf'] >= 3 and min(seen['asf'], seen['restore']) >= 100 and min(seen['ria'], seen['zero_weight']) >= 20, seen
    for e in (0, n - 1):
        assert np.array_equal(dev.get_cold(e), ora.get_cold(e)), e                   # the record itself, and everything around it
    dev.close(); ora.close()


def test_long_episodes_on_the_device():
    """Twelve-step episodes see few LocalWork failures: 24 episodes of 100 steps on the one-wave kernel, 90 steps in, against the host statement."""
    n, steps, seed = 24, 100, 8200
    dev = _dev(n, steps=steps, rng_mode=1, strict=False)
    dev.reset(seeds=seed)
    dev.enable_reward_terms()
    ria = lwf = 0
    for t in range(90):
        d = dev.step(U.blue_mix(seed, t, n))
        if t >= 30 and t % 3 == 0:
            terms, words = dev.reward_terms()
            ht, hw = U.from_rows(dev, range(n), steps)
            assert np.array_equal(terms, ht) and np.array_equal(words, hw), t
            U.check_identities(terms, words, d[1], t)
            ria += int((terms[..., 2] != 0).sum()); lwf += int((terms[..., 0] != 0).sum())
    assert ria >= 5 and lwf >= 20, (ria, lwf)
    dev.close()


def test_ids_banks_clones_faults_refusals_and_the_switch(monkeypatch):
    n, steps, seed = 64, 60, 8300
    monkeypatch.setenv('CC4_PHILOX_LEAN', '1')
    dev = _dev(n, steps=steps, rng_mode=1, strict=False)
    dev.reset(seeds=seed)
    lib, h = dev.lib, dev._h
    # the switch off: the fast builds record nothing
    dev.step(U.blue_mix(seed, 0, n))
    terms, words = dev.reward_terms()
    assert not terms.any() and (words[:, 0] == 0).all() and (words[:, 1] == 1).all() and not words[:, 3:].any()
    # the event log alone runs the full builds without records: nothing either
    dev.enable_event_log(True)
    dev.step(U.blue_mix(seed, 1, n))
    terms, words = dev.reward_terms()
    assert not terms.any() and (words[:, 0] == 0).all() and (words[:, 1] == 2).all() and not words[:, 3:].any()
    dev.enable_event_log(False)
    dev.enable_reward_terms()
    for t in range(2, 14):
        d = dev.step(U.blue_mix(seed, t, n))
    all_t, all_w = U.from_rows(dev, range(n), steps)
    U.check_identities(all_t, all_w, d[1], 'live')
    assert (all_w[:, 0] == 1).all() and (all_w[:, 1] == 14).all() and len({r.tobytes() for r in all_t}) >= 10 and (all_w[:, 4] != 0).sum() >= 5

    # shuffled, partial and duplicated id lists; the NumPy getter
    rng = np.random.default_rng(5)
    for ids in (rng.permutation(n), rng.permutation(n)[:3], rng.permutation(n)[:1], np.array([63, 0, 63, 31, 31])):
        ids = ids.astype(np.int32)
        terms, words = _view(dev, len(ids), ids=ids, fill=0x77)
        assert np.array_equal(terms, all_t[ids]) and np.array_equal(words, all_w[ids]), ids.tolist()
        terms, words = dev.reward_terms(ids)
        assert np.array_equal(terms, all_t[ids]) and np.array_equal(words, all_w[ids]), ids.tolist()
    terms, words = _view(dev, 3, ids=[7, 8, 9], fill=0x5A, words=False)              # no words wanted: their place stays as it was
    assert np.array_equal(terms, all_t[7:10]) and (words.view(np.uint8) == 0x5A).all()

    # episodes saved mid-episode into a bank and read in place, while the env steps on
    slot, cap = int(lib.cc4_snapshot_bytes(h)), 12
    bank = DevMem(cap * slot)
    src = np.array([3, 17, 40, 41, 63, 0, 9, 22], np.int32)
    dst = rng.permutation(8).astype(np.int32)
    idx = DevMem(4 * 32)
    idx.up(src); idx.up(dst, 64)
    assert lib.cc4_copy_episodes_device(h, len(src), None, 0, idx.p, bank.p, cap, idx.at(64), None) == 0, lib.cc4_last_error(h)
    # clone_episodes carries the record: episode 50 becomes episode 3
    dev.clone_episodes([3], [50])
    terms, words = dev.reward_terms([50, 3])
    assert np.array_equal(terms[0], all_t[3]) and np.array_equal(words[0], all_w[3]) and np.array_equal(terms[1], all_t[3])
    for t in range(14, 17):
        d = dev.step(U.blue_mix(seed, t, n))
    now_t, now_w = dev.reward_terms()
    assert (now_w[:, 1] == 17).all() and not np.array_equal(now_t[src], all_t[src])
    U.check_identities(now_t, now_w, d[1], 'after the clone')
    terms, words = _view(dev, len(dst), ids=dst, bank=bank, cap=cap)
    assert np.array_equal(terms, all_t[src]) and np.array_equal(words, all_w[src]) and all_t[src].any()
    terms, words = _view(dev, len(dst), bank=bank, cap=cap, words=False)             # no id list: slots 0 .. 7
    assert np.array_equal(terms, all_t[src[np.argsort(dst)]])
    assert _faults(dev) == 0

    # an id of -1, an id of N, a slot never written: zero rows, the other entries right, the fault in cc4_copy_faults
    by_slot = {int(d_): int(s_) for s_, d_ in zip(src, dst)}
    for bad_id, bit in ((10, CF_SLOT_EMPTY), (cap, CF_RANGE), (-1, CF_RANGE)):
        terms, words = _view(dev, 3, ids=[2, bad_id, 5], bank=bank, cap=cap, fill=0x77)
        assert not terms[1].any() and not words[1].any(), bad_id
        assert np.array_equal(terms[0], all_t[by_slot[2]]) and np.array_equal(terms[2], all_t[by_slot[5]]) and np.array_equal(words[2], all_w[by_slot[5]])
        assert _faults(dev) == bit, (bad_id, bit)
    terms, words = _view(dev, 4, ids=[n, 1, -1, 46], fill=0x77)
    assert not terms[0].any() and not terms[2].any() and not words[0].any() and not words[2].any()
    assert np.array_equal(terms[1], now_t[1]) and np.array_equal(terms[3], now_t[46]) and np.array_equal(words[3], now_w[46])
    assert _faults(dev) == CF_RANGE and _faults(dev) == 0
    with pytest.raises(Exception, match='INDEX_OUT_OF_RANGE'):
        dev.reward_terms([0, n])

    # refusals: -2, nothing enqueued, the output untouched; n = 0 a no-op
    out = DevMem(2 * (ROW_T + ROW_W), 0xC3)
    assert lib.cc4_reward_terms_device(h, None, 0, None, -1, out.p, out.at(2 * ROW_T)) == -2
    assert lib.cc4_reward_terms_device(h, None, 0, None, 2, None, out.at(2 * ROW_T)) == -2
    assert lib.cc4_reward_terms_device(h, None, 0, None, 2, out.at(8), out.at(2 * ROW_T)) == -2 and b'aligned' in lib.cc4_last_error(h)
    assert lib.cc4_reward_terms_device(h, None, 0, None, 2, out.p, out.at(2 * ROW_T + 4)) == -2 and b'aligned' in lib.cc4_last_error(h)
    assert lib.cc4_reward_terms_device(h, bank.p, 0, None, 2, out.p, out.at(2 * ROW_T)) == -2 and b'capacity' in lib.cc4_last_error(h)
    assert lib.cc4_reward_terms_device(h, None, 0, None, 0, out.p, out.at(2 * ROW_T)) == 0
    dev.synchronize()
    assert (out.down(np.uint8, out.nbytes) == 0xC3).all() and _faults(dev) == 0
    assert dev.reward_terms(np.zeros(0, np.int32))[0].shape == (0, 9, 4)
    # the calls that refuse a handle with submitted actions name the switch
    assert lib.cc4_rollout_begin(h, 4) == -2 and b'cc4_enable_reward_terms' in lib.cc4_last_error(h)
    assert lib.cc4_step_group_device(h, 0, None, None) == -2 and b'cc4_enable_reward_terms' in lib.cc4_last_error(h)

    # the switch off again: no action was ever submitted on this handle, it returns to the fast builds and the next step is not recorded
    dev.enable_reward_terms(False)
    assert not dev.reward_terms_enabled
    dev.step(U.blue_mix(seed, 17, n))
    terms, words = dev.reward_terms()
    assert not terms.any() and (words[:, 0] == 0).all() and (words[:, 1] == 18).all() and not words[:, 3:].any()
    # a handle that has taken a red action records with or without the switch, and never returns
    red = dev.agent_actions('red')
    d = dev.step_ex(U.blue_mix(seed, 18, n), None, red, None)
    dev.enable_reward_terms(False)
    d = dev.step(U.blue_mix(seed, 19, n))
    terms, words = dev.reward_terms()
    assert (words[:, 0] == 1).all() and (words[:, 1] == 20).all()
    U.check_identities(terms, words, d[1], 'after a submitted action')
    ht, hw = U.from_rows(dev, range(n), steps)
    assert np.array_equal(terms, ht) and np.array_equal(words, hw)
    for m in (bank, idx, out):
        m.free()
    dev.close()


@pytest.mark.parametrize('name,col,steps,nonzero', U.BRM_FIXTURES)
def test_the_blue_reward_machine_fixtures_on_the_numpy_stream_kernel(name, col, steps, nonzero):
    from cage_challenge_4_amd import CC4VecEnv
    fx = TS._load(name)
    n = nz = 0
    for case in fx['cases']:
        env = CC4VecEnv(1, steps=case['steps'], red_policy=case['red_policy'], green_policy=case['green_policy'])
        assert env.step_kernel == 'k_step'
        for k, e in enumerate(U.replay_scripted(env, case, TS._records)):
            terms, words = env.reward_terms()
            want = U.brm_cells(e, col)
            where = (name, case.get('note', ''), k)
            assert np.array_equal(terms[0], want), (where, terms[0].tolist(), want.tolist())
            assert words[0, 0] == 1 and words[0, 3] == e['expect']['brm'] and words[0, 3] + words[0, 4] == e['expect']['reward'], where
            ht, hw = RT.from_row(env.get_state(0), env.get_cold(0), case['steps'])
            assert np.array_equal(terms[0], ht) and np.array_equal(words[0], hw), where
            n += 1
            nz += e['expect']['brm'] != 0
        env.close()
    assert (n, nz) == (steps, nonzero)
