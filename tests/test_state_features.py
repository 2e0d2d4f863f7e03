"""GPU: k_state_features (cc4_state_features_device) against the host statement of the same definition (state_features.from_row of the
rows the handle returns) and, for a sample of episodes, against the independent derivation from the true-state document; its ordering behind
the group streams of a large batch; ids, snapshot banks, faults and refusals."""
import ctypes
import json

import numpy as np
import pytest

from cage_challenge_4_amd import state_features as SF
from cage_challenge_4_amd import true_state as T
from oracle_binding import OracleVecEnv, random_actions
from view_util import DevMem, _dev, _faults, call_view

pytestmark = pytest.mark.gpu

VP = ctypes.c_void_p
ROW_H, ROW_G = 137 * 16, 32 * 4
SE_ADD_RED_SESSION, SE_SET_RED_ACTIVE = 5, 9
CF_RANGE, CF_SLOT_EMPTY, CF_SLOT_CONFIG = 1, 8, 16


def _features(dev, n, ids=None, bank=None, cap=0, out=None, fill=0):
    """cc4_state_features_device into a fresh (or the given) device buffer [hosts | glob], then synchronise and copy down."""
    def call(d_bank, cap, d_ids, n, p_hosts, p_glob):
        assert dev.lib.cc4_state_features_device(dev._h, d_bank, cap, d_ids, n, p_hosts, p_glob) == 0, dev.lib.cc4_last_error(dev._h)
    return call_view(dev, call, n, ((np.uint8, (137, 16)), (np.int32, (32,))), ids, bank, cap, fill, out)


def _from_rows(rows):
    hg = [SF.from_row(r) for r in rows]
    return np.stack([h for h, _ in hg]), np.stack([g for _, g in hg])


def _long_lists(steps, rng_mode, seed):
    """An oracle episode with sessions added by hand (tests/test_red_wave_queries.py's pattern): ten on one host, root and not, of two agents."""
    ora = OracleVecEnv(1, steps=steps, rng_mode=rng_mode)
    ora.reset(seeds=seed)
    d = json.loads(ora.true_state_json(0))
    hosts = [h['h'] for h in d['hosts'] if h['h'] % 17 != 0 and h['h'] != 136]
    for j in range(10):
        assert ora.edit_state(0, SE_ADD_RED_SESSION, j % 2, hosts[3], (2 if j % 3 == 0 else 0) | (1 if j % 4 == 1 else 0)) >= 0
    for j in range(3):
        assert ora.edit_state(0, SE_ADD_RED_SESSION, 2, hosts[7], 2 | 4) >= 0
        assert ora.edit_state(0, SE_ADD_RED_SESSION, 3, hosts[11], 4) >= 0
    for r in range(4):
        ora.edit_state(0, SE_SET_RED_ACTIVE, r, 1)
    snap = ora.snapshot(0)
    ora.close()
    return snap, hosts[3]


@pytest.mark.parametrize('n,rng_mode,lean,kernel', [(65, 1, '0', 'k_step_philox'), (40, 1, '1', 'k_step_philox1'), (33, 0, None, 'k_step')],
                         ids=['4wave', '1wave', 'numpy_stream'])
def test_kernel_matches_host_function_on_every_episode(monkeypatch, n, rng_mode, lean, kernel):
    if lean is not None:
        monkeypatch.setenv('CC4_PHILOX_LEAN', lean)
    steps, seed = 30, 4100 + n
    dev = _dev(n, steps=steps, rng_mode=rng_mode, autoreset=True, strict=False)
    assert dev.step_kernel == kernel
    dev.reset(seeds=seed)
    edited = n - 2
    snap, crowded = _long_lists(steps, rng_mode, seed + 1)
    dev.restore(edited, snap)
    sample = sorted({0, 1, 2, n // 2, n - 3, edited, n - 1, 7})
    assert len(sample) == 8

    def check(what):
        hosts, glob = dev.state_features()
        assert hosts.shape == (n, 137, 16) and hosts.dtype == np.uint8 and glob.shape == (n, 32) and glob.dtype == np.int32
        want_h, want_g = _from_rows(dev.get_states())
        bad = np.argwhere(hosts != want_h)
        assert bad.size == 0, (what, [(int(e), int(h), int(c), int(hosts[e, h, c]), int(want_h[e, h, c])) for e, h, c in bad[:8]])
        assert np.array_equal(glob, want_g), (what, np.argwhere(glob != want_g)[:8].tolist())
        dev._chk(dev.lib.cc4_fetch(dev._h, *dev._p_out), 'cc4_fetch')
        for e in sample:
            th, tg = SF.from_true_state(T.decode(dev.true_state_json(e)), steps=steps, err=int(dev.err[e]))
            assert np.array_equal(hosts[e], th) and np.array_equal(glob[e], tg), (what, e)
        return hosts, glob

    hosts, glob = check('reset')
    assert hosts[edited, crowded, 4] >= 10 and hosts[edited, crowded, 2] == 2 and hosts[edited, crowded, 3] & 3 == 3      # the count and the root bit on the device
    assert (hosts[:, :, 0].sum(axis=1) > 20).all() and (glob[:, 1] == steps).all()
    t = 0
    while True:                                   # to the end of the episodes: all of them are truncated by the same step
        _o, _r, done, _i = dev.step(random_actions(seed, t, n))
        t += 1
        if t in (1, 2, 25):
            hosts, glob = check(t)
            assert (glob[:, 0] == t).all()
        if done.any():
            assert done.all() and t >= 25
            break
        assert t <= steps + 2
    hosts, glob = check('done')
    assert (glob[:, 3] == 1).all()
    dev.step(random_actions(seed, t, n))
    hosts, glob = check('regenerated')            # the step after `done` regenerated every episode
    assert (glob[:, 0] == 0).all() and (glob[:, 3] == 0).all()
    dev.close()


def test_call_is_ordered_behind_the_group_streams_of_a_large_batch():
    """6656 counter-mode episodes: a step is several launches on several streams, and calls of ten steps and more run the persistent kernel.
    run_random_steps(12), two cc4_step_device, then the features with no synchronise in between."""
    n, steps, seed0 = 6656, 200, 515
    dev = _dev(n, steps=steps, rng_mode=1, autoreset=True, strict=False)
    assert dev.launches_per_step > 1 and dev.run_kernel_for(12) == 'k_run_philox1' and dev.step_kernel == 'k_step_philox1'
    dev.reset(seeds=seed0)
    buf = DevMem(n * (ROW_H + ROW_G), 0xEE)
    acts = VP()
    dev._chk(dev.lib.cc4_actions_device(dev._h, ctypes.byref(acts)), 'cc4_actions_device')
    lib, h = dev.lib, dev._h
    dev.run_random_steps(seed0, 0, 12, timed=False)
    rc = lib.cc4_step_device(h, acts, None) or lib.cc4_step_device(h, acts, None)
    rc = rc or lib.cc4_state_features_device(h, None, 0, None, n, buf.p, buf.at(n * ROW_H))
    assert rc == 0, lib.cc4_last_error(h)
    dev.synchronize()
    hosts, glob = buf.down(np.uint8, (n, 137, 16)), buf.down(np.int32, (n, 32), n * ROW_H)
    want_h, want_g = _from_rows(dev.get_states())
    assert (want_g[:, 0] == 14).all()
    bad = sorted(set(np.argwhere(hosts != want_h)[:, 0].tolist()) | set(np.argwhere(glob != want_g)[:, 0].tolist()))
    assert not bad, (len(bad), bad[:10])
    buf.free()
    dev.close()


def test_ids_banks_faults_and_refusals():
    n, steps = 48, 30
    dev = _dev(n, steps=steps, rng_mode=1, strict=False)
    dev.reset(seeds=88)
    for t in range(5):
        dev.step(random_actions(88, t, n))
    lib, h = dev.lib, dev._h
    all_h, all_g = dev.state_features()
    assert np.array_equal(all_h, _from_rows(dev.get_states())[0])
    # a shuffled id list with duplicates: rows in the order asked for
    rng = np.random.default_rng(3)
    ids = np.concatenate([rng.permutation(n)[:20], [5, 5, 47, 0, 5]]).astype(np.int32)
    hosts, glob = _features(dev, len(ids), ids=ids)
    assert np.array_equal(hosts, all_h[ids]) and np.array_equal(glob, all_g[ids])
    hosts, glob = dev.state_features(ids[:7])
    assert np.array_equal(hosts, all_h[ids[:7]]) and np.array_equal(glob, all_g[ids[:7]])
    # n = 0: a no-op
    canary = DevMem(ROW_H + ROW_G, 0xC3)
    assert lib.cc4_state_features_device(h, None, 0, None, 0, canary.p, canary.at(ROW_H)) == 0
    dev.synchronize()
    assert (canary.down(np.uint8, canary.nbytes) == 0xC3).all()
    assert dev.state_features(np.zeros(0, np.int32))[0].shape == (0, 137, 16)

    # 16 episodes into a bank; the env steps on; the bank's slots still show the state at the save
    slot, cap = int(lib.cc4_snapshot_bytes(h)), 20
    bank = DevMem(cap * slot)
    src = np.arange(3, 3 + 16, dtype=np.int32)
    dst = rng.permutation(16).astype(np.int32)
    idx = DevMem(4 * 32)
    idx.up(src); idx.up(dst, 64)
    assert lib.cc4_copy_episodes_device(h, 16, None, 0, idx.p, bank.p, cap, idx.at(64), None) == 0, lib.cc4_last_error(h)
    for t in range(5, 8):
        dev.step(random_actions(88, t, n))
    now_h, now_g = dev.state_features()
    assert (now_g[:, 0] == 8).all() and not np.array_equal(now_h[src], all_h[src])
    hosts, glob = _features(dev, 16, ids=dst, bank=bank, cap=cap)
    assert np.array_equal(hosts, all_h[src]) and np.array_equal(glob, all_g[src])
    inv = np.argsort(dst)
    hosts, glob = _features(dev, 16, bank=bank, cap=cap)              # no id list: slots 0 .. 15
    assert np.array_equal(hosts, all_h[src[inv]]) and np.array_equal(glob, all_g[src[inv]])
    assert _faults(dev) == 0

    # a slot written by a handle of another episode length: its header and the head of its row into slot 18
    other = _dev(2, steps=steps + 10, rng_mode=1)
    other.reset(seeds=9)
    oslot = int(other.lib.cc4_snapshot_bytes(other._h))
    obank = DevMem(oslot)
    zero = DevMem(16)
    assert other.lib.cc4_copy_episodes_device(other._h, 1, None, 0, zero.p, obank.p, 1, zero.p, None) == 0
    other.synchronize()
    head = obank.down(np.uint8, min(slot, oslot))
    bank.up(head, 18 * slot)
    other.close()
    # each fault alone: an all-zero row and its bit; then together, the other rows of the call correct
    by_slot = {int(d): int(s) for s, d in zip(src, dst)}
    for bad_id, bit in ((17, CF_SLOT_EMPTY), (cap, CF_RANGE), (-1, CF_RANGE), (18, CF_SLOT_CONFIG)):
        hosts, glob = _features(dev, 3, ids=[2, bad_id, 9], bank=bank, cap=cap, fill=0x77)
        assert not hosts[1].any() and not glob[1].any(), bad_id
        assert np.array_equal(hosts[0], all_h[by_slot[2]]) and np.array_equal(hosts[2], all_h[by_slot[9]]) and np.array_equal(glob[2], all_g[by_slot[9]])
        assert _faults(dev) == bit, (bad_id, bit)
    hosts, glob = _features(dev, 4, ids=[n, 1, -5, 46], fill=0x77)      # the handle's own episodes: ids past the batch
    assert not hosts[0].any() and not hosts[2].any() and not glob[0].any() and not glob[2].any()
    assert np.array_equal(hosts[1], now_h[1]) and np.array_equal(hosts[3], now_h[46]) and np.array_equal(glob[3], now_g[46])
    assert _faults(dev) == CF_RANGE and _faults(dev) == 0
    hosts, glob = _features(dev, 5, ids=[17, 0, 18, 19, cap + 3], bank=bank, cap=cap, fill=0x77)
    assert not hosts[[0, 2, 3, 4]].any() and not glob[[0, 2, 3, 4]].any() and np.array_equal(hosts[1], all_h[by_slot[0]])
    assert _faults(dev) == CF_RANGE | CF_SLOT_EMPTY | CF_SLOT_CONFIG
    with pytest.raises(Exception, match='INDEX_OUT_OF_RANGE'):
        dev.state_features([0, n])

    # refusals: -2, nothing enqueued, the output untouched
    out = DevMem(2 * (ROW_H + ROW_G), 0xC3)
    assert lib.cc4_state_features_device(h, None, 0, None, -1, out.p, out.at(2 * ROW_H)) == -2
    assert lib.cc4_state_features_device(h, None, 0, None, 2, None, out.at(2 * ROW_H)) == -2
    assert lib.cc4_state_features_device(h, None, 0, None, 2, out.at(4), out.at(2 * ROW_H)) == -2 and b'aligned' in lib.cc4_last_error(h)
    assert lib.cc4_state_features_device(h, bank.p, 0, None, 2, out.p, out.at(2 * ROW_H)) == -2 and b'capacity' in lib.cc4_last_error(h)
    assert lib.cc4_state_features_device(h, bank.p, -3, None, 2, out.p, out.at(2 * ROW_H)) == -2
    dev.synchronize()
    assert (out.down(np.uint8, out.nbytes) == 0xC3).all() and _faults(dev) == 0
    assert lib.cc4_state_features_device(h, None, 0, None, 2, out.p, None) == 0          # the episode words are optional
    dev.synchronize()
    assert np.array_equal(out.down(np.uint8, (2, 137, 16)), now_h[:2]) and (out.down(np.uint8, 2 * ROW_G, 2 * ROW_H) == 0xC3).all()
    for m in (canary, bank, idx, obank, zero, out):
        m.free()
    dev.close()


def test_refused_while_a_rollout_is_in_flight():
    n, K = 8192, 4
    dev = _dev(n, steps=50, rng_mode=1)
    dev.reset(seeds=4)
    lib, h = dev.lib, dev._h
    out = DevMem(2 * (ROW_H + ROW_G), 0xC3)
    assert lib.cc4_rollout_begin(h, K) == 0, lib.cc4_last_error(h)
    assert lib.cc4_state_features_device(h, None, 0, None, 2, out.p, out.at(2 * ROW_H)) == -2 and b'rollout' in lib.cc4_last_error(h)
    G_, blk = ctypes.c_int32(), ctypes.c_int32()
    rc = lib.cc4_rollout_groups(h, ctypes.byref(G_), ctypes.byref(blk))
    s0 = ctypes.c_uint64(4)
    for j in range(K):
        for g in range(G_.value):
            rc = rc or lib.cc4_rollout_sync(h, g if j > 0 else -1, j - 1, g, j, None)
            rc = rc or lib.cc4_rollout_random_policy(h, g, j, s0, ctypes.c_uint32(j), None)
    for g in range(G_.value):
        rc = rc or lib.cc4_rollout_sync(h, g, K - 1, -1, 0, None)
    assert lib.cc4_rollout_end(h) == 0 and rc == 0, lib.cc4_last_error(h)
    assert (out.down(np.uint8, out.nbytes) == 0xC3).all()
    assert lib.cc4_state_features_device(h, None, 0, None, 2, out.p, out.at(2 * ROW_H)) == 0          # after the rollout: fine
    dev.synchronize()
    want_h, want_g = _from_rows([dev.get_state(0), dev.get_state(1)])
    assert np.array_equal(out.down(np.uint8, (2, 137, 16)), want_h) and np.array_equal(out.down(np.int32, (2, 32), 2 * ROW_H), want_g)
    assert (want_g[:, 0] == K).all()
    out.free()
    dev.close()
