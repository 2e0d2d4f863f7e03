"""GPU: blue's own knowledge from the device.  cc4_blue_view_device (k_blue_view) against the view derived from the REFERENCE's dict observation
(tests/blue_util.py) on the 120 recorded steps of blueobs_seed123_random.json, and against the host statement of the same definition
(blue_view.from_row) byte for byte on a batch with the event log on: id lists whose odd output indices give blocks that are not 16-byte aligned,
snapshot banks, no agent words, faults, refusals; and the same handle with the log off."""
import ctypes
import json
import os

import numpy as np
import pytest

import blue_util as BU
import golden_util
from cage_challenge_4_amd import blue_view as BV
from oracle_binding import random_actions
from view_util import DevMem, _dev, _faults, call_view

pytestmark = pytest.mark.gpu

VP = ctypes.c_void_p
ROW_H, ROW_S = 5 * 137 * 8, 5 * 16 * 4
CF_RANGE, CF_SLOT_EMPTY = 1, 8


def _view(dev, n, ids=None, bank=None, cap=0, fill=0, scalars=True):
    """cc4_blue_view_device into a fresh device buffer [hosts | scalars], then synchronise and copy down."""
    def call(d_bank, cap, d_ids, n, p_hosts, p_scal):
        dev.blue_view_device(p_hosts, p_scal, n=n, d_ids=d_ids, d_bank=d_bank, capacity=cap)
    return call_view(dev, call, n, ((np.uint8, (5, 137, 8)), (np.int32, (5, 16))), ids, bank, cap, fill, second=scalars)


def _from_rows(dev, episodes, steps):
    hs = [BV.from_row(dev.get_state(e), dev.get_cold(e), steps) for e in episodes]
    return np.stack([h for h, _ in hs]), np.stack([s for _, s in hs])


def test_device_view_matches_the_reference_dict_observation():
    """(a) One episode on the numpy stream, the reference's own trajectory: the kernel's view of each of the 120 recorded steps against the view
    derived from the reference's dict observation of that step."""
    gold = json.load(open(os.path.join(golden_util.GOLDEN_DIR, 'blueobs_seed123_random.json')))
    fix = golden_util.load(os.path.join(golden_util.GOLDEN_DIR, gold['fixture']))
    dev = _dev(1, steps=fix['steps'])
    dev.reset(seeds=fix['seed'])
    dev.reset(seeds=None)
    dev.enable_event_log(True)
    stats = BU.new_stats()
    for t, want in enumerate(gold['steps']):
        dev.step(fix['actions'][t][None, :])
        hosts, scal = dev.blue_view()
        assert hosts.shape == (1, 5, 137, 8) and hosts.dtype == np.uint8 and scal.shape == (1, 5, 16) and scal.dtype == np.int32
        assert (scal[0, :, 10] == 1).all() and (scal[0, :, 13] == t + 1).all(), t
        BU.compare(hosts[0], scal[0], want, json.loads(dev.true_state_json(0)), t, stats)
    assert stats['pairs'] >= 550 and stats['files'] >= 10 and stats['decoys'] >= 30, stats
    dev.close()


def test_device_view_equals_the_host_function_with_ids_banks_faults_and_the_log_off():
    n, steps, seed, T = 64, 60, 4700, 40
    dev = _dev(n, steps=steps, rng_mode=1, strict=False)
    dev.reset(seeds=seed)
    dev.enable_event_log(True)
    lib, h = dev.lib, dev._h
    everyone = range(n)
    seen = dict(busy=0, own=0, conn=0, remote_outside=0, sus=0, success=set())
    all_h = all_s = None
    for t in range(T):
        dev.step(random_actions(seed, t, n))
        if t % 5 == 4:
            hosts, scal = dev.blue_view()
            all_h, all_s = _from_rows(dev, everyone, steps)
            bad = np.argwhere(hosts != all_h)
            assert bad.size == 0, (t, [tuple(map(int, b)) + (int(hosts[tuple(b)]), int(all_h[tuple(b)])) for b in bad[:8]])
            assert np.array_equal(scal, all_s), (t, np.argwhere(scal != all_s)[:8].tolist())
            assert (scal[..., 10] == 1).all() and (scal[..., 13] == t + 1).all(), t
            seen['busy'] += int(scal[..., 0].sum()); seen['own'] += int((hosts[..., 7] != 0).sum()); seen['conn'] += int(hosts[..., 3].astype(np.int64).sum())
            seen['remote_outside'] += int((hosts[..., 5][hosts[..., 0] == 0] != 0).sum()); seen['sus'] += int((hosts[..., 2] != 0).sum())
            seen['success'] |= set(np.unique(scal[..., 7]).tolist())
    assert seen['busy'] > 0 and seen['own'] > 0 and seen['conn'] > 100 and seen['remote_outside'] > 0 and seen['sus'] > 0, seen
    assert {BV.T_TRUE, BV.T_UNKNOWN, BV.T_IN_PROGRESS} <= seen['success'], seen

    # shuffled id lists of 3 and of 1: output index 1 of three starts at byte 5480, 8- but not 16-byte aligned
    rng = np.random.default_rng(5)
    for ids in (rng.permutation(n)[:3], rng.permutation(n)[:1], np.array([63, 0, 63, 31, 31], np.int64)):
        ids = ids.astype(np.int32)
        hosts, scal = _view(dev, len(ids), ids=ids, fill=0x77)
        assert np.array_equal(hosts, all_h[ids]) and np.array_equal(scal, all_s[ids]), ids.tolist()
        hosts, scal = dev.blue_view(ids)
        assert np.array_equal(hosts, all_h[ids]) and np.array_equal(scal, all_s[ids]), ids.tolist()
    # no agent words wanted: the words' place stays as it was
    hosts, scal = _view(dev, 3, ids=[7, 8, 9], fill=0x5A, scalars=False)
    assert np.array_equal(hosts, all_h[7:10]) and (scal.view(np.uint8) == 0x5A).all()

    # episodes into a bank: the view from the bank equals the live one; the env steps on and the slots still show the view at the save
    slot, cap = int(lib.cc4_snapshot_bytes(h)), 12
    bank = DevMem(cap * slot)
    src = np.array([3, 17, 40, 41, 63, 0, 9, 22], np.int32)
    dst = rng.permutation(8).astype(np.int32)
    idx = DevMem(4 * 32)
    idx.up(src); idx.up(dst, 64)
    assert lib.cc4_copy_episodes_device(h, len(src), None, 0, idx.p, bank.p, cap, idx.at(64), None) == 0, lib.cc4_last_error(h)
    hosts, scal = _view(dev, len(dst), ids=dst, bank=bank, cap=cap)
    assert np.array_equal(hosts, all_h[src]) and np.array_equal(scal, all_s[src])
    assert all_h[src][..., 3:7].any() and all_h[src][..., 2].any()                  # the log and the sus lists travelled with the copy
    for t in range(T, T + 3):
        dev.step(random_actions(seed, t, n))
    now_h, now_s = dev.blue_view()
    assert (now_s[..., 13] == T + 3).all() and not np.array_equal(now_h[src], all_h[src])
    hosts, scal = _view(dev, len(dst), ids=dst, bank=bank, cap=cap)
    assert np.array_equal(hosts, all_h[src]) and np.array_equal(scal, all_s[src])
    inv = np.argsort(dst)
    hosts, scal = _view(dev, len(dst), bank=bank, cap=cap, scalars=False)          # no id list: slots 0 .. 7
    assert np.array_equal(hosts, all_h[src[inv]])
    assert _faults(dev) == 0

    # an id of -1, an id of N, a slot never written: zero rows, the other entries right, the fault in cc4_copy_faults
    by_slot = {int(d): int(s) for s, d in zip(src, dst)}
    for bad_id, bit in ((10, CF_SLOT_EMPTY), (cap, CF_RANGE), (-1, CF_RANGE)):
        hosts, scal = _view(dev, 3, ids=[2, bad_id, 5], bank=bank, cap=cap, fill=0x77)
        assert not hosts[1].any() and not scal[1].any(), bad_id
        assert np.array_equal(hosts[0], all_h[by_slot[2]]) and np.array_equal(hosts[2], all_h[by_slot[5]]) and np.array_equal(scal[2], all_s[by_slot[5]])
        assert _faults(dev) == bit, (bad_id, bit)
    hosts, scal = _view(dev, 4, ids=[n, 1, -1, 46], fill=0x77)
    assert not hosts[0].any() and not hosts[2].any() and not scal[0].any() and not scal[2].any()
    assert np.array_equal(hosts[1], now_h[1]) and np.array_equal(hosts[3], now_h[46]) and np.array_equal(scal[3], now_s[46])
    assert _faults(dev) == CF_RANGE and _faults(dev) == 0
    with pytest.raises(Exception, match='INDEX_OUT_OF_RANGE'):
        dev.blue_view([0, n])

    # refusals: -2, nothing enqueued, the output untouched; n = 0 a no-op
    out = DevMem(2 * (ROW_H + ROW_S), 0xC3)
    assert lib.cc4_blue_view_device(h, None, 0, None, -1, out.p, out.at(2 * ROW_H)) == -2
    assert lib.cc4_blue_view_device(h, None, 0, None, 2, None, out.at(2 * ROW_H)) == -2
    assert lib.cc4_blue_view_device(h, None, 0, None, 2, out.at(4), out.at(2 * ROW_H)) == -2 and b'aligned' in lib.cc4_last_error(h)
    assert lib.cc4_blue_view_device(h, bank.p, 0, None, 2, out.p, out.at(2 * ROW_H)) == -2 and b'capacity' in lib.cc4_last_error(h)
    assert lib.cc4_blue_view_device(h, None, 0, None, 0, out.p, out.at(2 * ROW_H)) == 0
    dev.synchronize()
    assert (out.down(np.uint8, out.nbytes) == 0xC3).all() and _faults(dev) == 0
    assert dev.blue_view(np.zeros(0, np.int32))[0].shape == (0, 5, 137, 8)
    assert lib.cc4_blue_view_device(h, None, 0, None, 1, out.at(8), out.at(2 * ROW_H)) == 0          # 8-byte alignment is what the kernel needs
    dev.synchronize()
    assert np.array_equal(out.down(np.uint8, (1, 5, 137, 8), 8), now_h[:1])

    # (c) the same handle with the log off: events_valid 0, no event columns, everything else as the host function states it
    dev.enable_event_log(False)
    for t in range(T + 3, T + 6):
        dev.step(random_actions(seed, t, n))
    hosts, scal = dev.blue_view()
    off_h, off_s = _from_rows(dev, everyone, steps)
    assert np.array_equal(hosts, off_h) and np.array_equal(scal, off_s)
    assert (scal[..., 10] == 0).all() and (scal[..., 11] == 0).all() and not hosts[..., 3:7].any() and not (hosts[..., 7] & BV.OWN_DECOY).any()
    assert hosts[..., 0].any() and hosts[..., 2].any() and (scal[..., 13] == T + 6).all() and (scal[..., 0] == 1).any()
    hot_h, hot_s = zip(*[BV.from_row(dev.get_state(e)) for e in everyone])          # the hot row alone
    keep = [k for k in range(16) if k not in (10, 11)]
    assert np.array_equal(hosts[..., [0, 1, 7]], np.stack(hot_h)[..., [0, 1, 7]]) and np.array_equal(scal[..., keep], np.stack(hot_s)[..., keep])
    for m in (bank, idx, out):
        m.free()
    dev.close()
