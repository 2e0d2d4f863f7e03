"""GPU: masked sampling of the blue actions from policy logits on the device.  cc4_sample_actions_device (k_sample_actions) against the host
statement of the same definition (action_sampling.from_row) on the rows cc4_get_state returns and against the float64 restatement
(action_sampling.reference), over the three logits dtypes, sampled and greedy, two temperatures, both busy settings and no logits; the crafted
logits at the segment edges, where a lane-to-slot mapping goes wrong; id lists and a snapshot bank; faults and refusals; and the distribution of
the draws over 256 clones of one episode.  The tolerances: sample_util (the kernel and the host function are both float32, on two libms)."""
import ctypes

import numpy as np
import pytest

import sample_util as U
from cage_challenge_4_amd import action_sampling as AS
from view_util import DevMem, _dev, _faults, call_view

pytestmark = pytest.mark.gpu

VP = ctypes.c_void_p
CF_RANGE, CF_SLOT_EMPTY = 1, 8
STEPS = 30
SEG = np.array(AS.SEGMENTS[:5])


def _sample(dev, n, logits=None, code=3, seed=0, t=0, T=1.0, flags=AS.BUSY, ids=None, bank=None, cap=0, fill=0x77, stats=True):
    """cc4_sample_actions_device into a fresh device buffer [actions | stats], then synchronise and copy down.  logits: the array to hand the
    device ([n, 570] float32 / float16 / uint16 bfloat16 patterns) or None."""
    d_lg = None
    if logits is not None:
        logits = np.ascontiguousarray(logits)
        assert logits.shape == (n, 570) and logits.dtype.itemsize == (4 if code == 3 else 2)
        d_lg = DevMem(logits.nbytes)
        d_lg.up(logits)

    def call(d_bank, cap_, d_ids, n_, p_act, p_st):
        dev.sample_actions_device(p_act, p_st, d_lg.p if d_lg else None, code, seed, t, T, flags, n=n_, d_ids=d_ids, d_bank=d_bank, capacity=cap_)
    out = call_view(dev, call, n, ((np.int32, (5,)), (np.float32, (5, 2))), ids, bank, cap, fill, second=stats)
    if d_lg:
        d_lg.free()
    return out


def _stepped(n, seed, steps=6):
    """A counter-mode env stepped `steps` steps with sampled actions in which some agents submit a Restore, so that busy agents exist."""
    dev = _dev(n, steps=STEPS, rng_mode=1, strict=False)
    dev.reset(seeds=seed)
    mask = dev.action_mask
    for t in range(steps):
        act, _ = _sample(dev, n, seed=77, t=t)
        for e in range(n):
            for b in range(5):
                if (e + b + t) % 3 == 0 and act[e, b] >= 0:
                    act[e, b] = 2 * (16 if b < 4 else 48) + 1 + U.valid_slots(mask[e], b)[0]
        dev.step(act)
    return dev, mask


@pytest.mark.parametrize('n', [3, 65])
def test_kernel_against_the_host_function_and_the_restatement(n):
    """(a) 65 entries: one workgroup index beyond a wave's lane count."""
    dev, mask = _stepped(n, 300 + n)
    hots = dev.get_states()
    busy = [U.busy_of(h, STEPS) for h in hots]
    assert any(b.any() for b in busy) and not all(b.all() for b in busy)
    rng = np.random.default_rng(n)
    base = U.random_logits(rng, (n, 570))
    tally = U.Tally()
    t = 11
    for code, (vals, dev_arr) in U.value_sets(base).items():
        for greedy in (False, True):
            for T in (1.0, 0.5):
                for busy_aware in (True, False):
                    flags = AS.flags_of(greedy, busy_aware)
                    act, st = _sample(dev, n, dev_arr, code, 5, t, T, flags)
                    for e in range(n):
                        what = f'dtype {code} greedy {greedy} T {T} busy_aware {busy_aware} entry {e}'
                        ha, hs, refused = AS.from_row(hots[e], vals[e], 5, t, e, T, greedy, busy_aware)
                        ref = AS.reference(mask[e], busy[e], vals[e], 5, t, e, T, greedy, busy_aware, details=True)
                        assert not refused
                        tally.check(act[e], st[e], ref, what)
                        sure = ref[3] >= 2.0 ** -12 * ref[4]['zmax']
                        assert np.array_equal(act[e][sure], ha[sure]), what                 # ... and so the host function's
                        same = act[e] == ha
                        assert np.abs(st[e][same] - hs[same]).max(initial=0.0) <= 2.0 ** -12 * max(1.0, np.abs(hs).max()), what
                        if busy_aware:
                            assert ((act[e] == -1) == busy[e]).all() and not st[e][busy[e]].any(), what
                        ok = act[e] >= 0
                        assert mask[e][SEG[ok] + act[e][ok]].all(), what
    # no logits: uniform over the valid slots; greedy without logits is all ties: the lowest valid slot
    act, st = _sample(dev, n, None, 3, 5, t, 1.0, 0)
    for e in range(n):
        tally.check(act[e], st[e], AS.reference(mask[e], busy[e], None, 5, t, e, 1.0, False, False, details=True), f'no logits, entry {e}')
        nvalid = np.array([U.valid_slots(mask[e], b).size for b in range(5)])
        assert np.allclose(st[e, :, 0], -np.log(nvalid), atol=2.0 ** -12 * 6) and np.allclose(st[e, :, 1], np.log(nvalid), atol=2.0 ** -12 * 6)
    act, _ = _sample(dev, n, None, 1, 5, t, 0.5, AS.GREEDY)
    assert np.array_equal(act, [[U.valid_slots(mask[e], b)[0] for b in range(5)] for e in range(n)])
    tally.close(f'kernel against the restatement, N = {n}')
    # without the second output the stats' place stays as it was
    act2, guard = _sample(dev, n, base, 3, 5, t, 1.0, 0, fill=0x5A, stats=False)
    act3, _ = _sample(dev, n, base, 3, 5, t, 1.0, 0)
    assert np.array_equal(act2, act3) and (guard.view(np.uint8) == 0x5A).all()
    assert _faults(dev) == 0
    dev.close()


def test_crafted_logits_at_the_segment_edges_ids_and_a_bank():
    """(b) the crafted logits of the CPU test at N = 3; (c) shuffled and repeated ids, and a bank read in place."""
    n = 3
    seed = U.edge_seed(1, STEPS)
    dev = _dev(n, steps=STEPS, rng_mode=1, strict=False)
    dev.reset(seeds=seed)
    mask = dev.action_mask
    m = mask[0]
    rows = U.crafted_edge_rows(m)
    for code in (3, 2, 1):
        for name, lg, b, k in rows:
            arr = U.value_sets(np.tile(lg, (n, 1)))[code][1]          # (+-20 is exact in all three)
            for t in range(2):
                act, st = _sample(dev, n, arr, code, 9, t, 1.0, 0)
                assert act[0, b] == k and abs(st[0, b, 0]) < 2.0 ** -12, (code, name, t, act[0].tolist())
    rng = np.random.default_rng(3)
    base = U.random_logits(rng, (n, 570))
    want_a, want_s = _sample(dev, n, base, 3, 9, 1, 1.0, 0)
    # 3e38 and NaN on invalid slots only: no effect, no fault
    lg = base.copy()
    for e in range(n):
        inv = np.nonzero(~mask[e])[0]
        lg[e, inv[::2]], lg[e, inv[1::2]] = 3e38, np.nan
    act, st = _sample(dev, n, lg, 3, 9, 1, 1.0, 0)
    assert np.array_equal(act, want_a) and np.array_equal(st, want_s) and _faults(dev) == 0
    # -inf on all valid slots but one: that one is drawn, with logp = 0
    lg = base.copy()
    keep = np.array([[U.valid_slots(mask[e], b)[-1] for b in range(5)] for e in range(n)])
    lg[mask] = -np.inf
    for e in range(n):
        lg[e, SEG + keep[e]] = base[e, SEG + keep[e]]
    for flags in (0, AS.GREEDY):
        act, st = _sample(dev, n, lg, 3, 9, 1, 0.5, flags)
        assert np.array_equal(act, keep) and not st.any() and _faults(dev) == 0
    # NaN / +inf on a valid slot, all valid slots -inf: CF_RANGE, only that agent at -1
    for b, poison in ((0, 'nan'), (4, 'nan'), (2, 'inf'), (3, '-inf')):
        lg = base.copy()
        v = U.valid_slots(mask[1], b)
        if poison == '-inf':
            lg[1, SEG[b] + v] = -np.inf
        else:
            lg[1, SEG[b] + v[-1]] = np.nan if poison == 'nan' else np.inf
        act, st = _sample(dev, n, lg, 3, 9, 1, 1.0, 0)
        assert act[1, b] == -1 and not st[1, b].any(), (b, poison)
        want = want_a.copy(); want[1, b] = -1
        wst = want_s.copy(); wst[1, b] = 0
        assert np.array_equal(act, want) and np.array_equal(st, wst), (b, poison)
        assert _faults(dev) == CF_RANGE and _faults(dev) == 0

    # (c) ids: the rows of those episodes, the noise of those episodes -- independent of the order
    hots = dev.get_states()
    for ids in ([2, 0, 1], [1, 1, 2, 0, 1], [2]):
        k = len(ids)
        lg = U.random_logits(rng, (k, 570))
        act, st = _sample(dev, k, lg, 3, 9, 4, 1.0, AS.BUSY, ids=ids)
        for j, e in enumerate(ids):
            ha, hs, _ = AS.from_row(hots[e], lg[j], 9, 4, e)
            assert np.array_equal(act[j], ha) and np.abs(st[j] - hs).max() <= 2.0 ** -12 * max(1.0, np.abs(hs).max()), (ids, j)
    same = np.tile(base[:1], (5, 1))
    act, st = _sample(dev, 5, same, 3, 9, 4, 1.0, 0, ids=[1, 1, 2, 0, 1])
    assert np.array_equal(act[0], act[1]) and np.array_equal(act[0], act[4]) and np.array_equal(st[0], st[4])
    # a bank: the live episodes' results where the slot id equals the episode id
    lib, h = dev.lib, dev._h
    slot, cap = int(lib.cc4_snapshot_bytes(h)), 4
    bank = DevMem(cap * slot)
    idx = DevMem(64)
    idx.up(np.arange(n, dtype=np.int32))
    assert lib.cc4_copy_episodes_device(h, n, None, 0, idx.p, bank.p, cap, idx.p, None) == 0, lib.cc4_last_error(h)
    live = _sample(dev, n, base, 3, 9, 4, 1.0, AS.BUSY)
    banked = _sample(dev, n, base, 3, 9, 4, 1.0, AS.BUSY, bank=bank, cap=cap, ids=[0, 1, 2])
    assert np.array_equal(live[0], banked[0]) and np.array_equal(live[1], banked[1]) and _faults(dev) == 0

    # (d) faults: an id out of range and a never-written slot give -1 rows and zero stats, the other entries right
    for bad_id, bit in ((3, CF_SLOT_EMPTY), (cap, CF_RANGE), (-1, CF_RANGE)):
        act, st = _sample(dev, 3, base, 3, 9, 4, 1.0, AS.BUSY, bank=bank, cap=cap, ids=[0, bad_id, 2])
        assert (act[1] == -1).all() and not st[1].any() and np.array_equal(act[[0, 2]], live[0][[0, 2]]) and np.array_equal(st[[0, 2]], live[1][[0, 2]])
        assert _faults(dev) == bit and _faults(dev) == 0, bad_id
    act, st = _sample(dev, 3, base, 3, 9, 4, 1.0, AS.BUSY, ids=[0, n, 2])
    assert (act[1] == -1).all() and not st[1].any() and np.array_equal(act[0], live[0][0]) and _faults(dev) == CF_RANGE
    with pytest.raises(Exception, match='INDEX_OUT_OF_RANGE'):
        dev.sample_actions(base, ids=[0, n, 2])
    a_np, s_np = dev.sample_actions(base, seed=9, t=4)
    assert np.array_equal(a_np, live[0]) and np.array_equal(s_np, live[1])
    bad = base.copy()
    bad[1, SEG[0] + U.valid_slots(mask[1], 0)[0]] = np.nan
    with pytest.raises(Exception, match='INDEX_OUT_OF_RANGE'):
        dev.sample_actions(bad)

    # refusals of the entry point's own: -2 with a message, nothing enqueued, the outputs untouched; n = 0 a no-op
    out = DevMem(3 * 20 + 3 * 40, 0xC3)
    d_lg = DevMem(base.nbytes + 16)
    d_lg.up(base)
    d_st = out.at(60)
    f = ctypes.c_float
    call = lambda n_=3, dt=3, lg=d_lg.p, T=1.0, fl=0, pa=out.p, ps=d_st, bk=None, cp=0: lib.cc4_sample_actions_device(h, bk, cp, None, n_, dt, lg, 9, 4, f(T), fl, pa, ps)      # noqa: E731
    for kw, word in ((dict(dt=0), b'dtype'), (dict(dt=4), b'dtype'), (dict(T=0.0), b'temperature'), (dict(T=-1.0), b'temperature'),
                     (dict(T=float('nan')), b'temperature'), (dict(T=float('inf')), b'temperature'), (dict(fl=4), b'flag'), (dict(fl=-1), b'flag'),
                     (dict(lg=d_lg.at(2)), b'aligned'), (dict(n_=-1), b'n < 0'), (dict(pa=None), b'aligned'), (dict(pa=out.at(2)), b'aligned'),
                     (dict(ps=out.at(62)), b'aligned'), (dict(bk=bank.p, cp=0), b'capacity')):
        assert call(**kw) == -2 and word in lib.cc4_last_error(h), (kw, lib.cc4_last_error(h))
    assert call(n_=0) == 0
    dev.synchronize()
    assert (out.down(np.uint8, out.nbytes) == 0xC3).all() and _faults(dev) == 0
    # the handle's own action buffer is a legal destination: sample straight into what cc4_step_device reads
    p_act = VP()
    assert lib.cc4_actions_device(h, ctypes.byref(p_act)) == 0
    assert call(pa=p_act, ps=None, fl=AS.BUSY) == 0
    got = np.zeros((n, 5), np.int32)
    assert lib.cc4_get_actions(h, got.ctypes.data_as(VP)) == 0 and np.array_equal(got, live[0])
    for mobj in (bank, idx, out, d_lg):
        mobj.free()
    dev.close()


def test_refused_while_a_rollout_is_in_flight():
    n, K = 8192, 2
    dev = _dev(n, steps=50, rng_mode=1)
    dev.reset(seeds=4)
    lib, h = dev.lib, dev._h
    out = DevMem(2 * 60, 0xC3)
    call = lambda: lib.cc4_sample_actions_device(h, None, 0, None, 2, 3, None, 1, 2, ctypes.c_float(1.0), 0, out.p, out.at(40))      # noqa: E731
    assert lib.cc4_rollout_begin(h, K) == 0, lib.cc4_last_error(h)
    assert call() == -2 and b'rollout' in lib.cc4_last_error(h)
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
    assert call() == 0          # after the rollout: fine
    dev.synchronize()
    for e in range(2):
        ha, hs, _ = AS.from_row(dev.get_state(e), None, 1, 2, e, 1.0, False, False)
        assert np.array_equal(out.down(np.int32, (2, 5))[e], ha)
    out.free()
    dev.close()


def test_distribution_on_the_device():
    """(e) 256 clones of one episode, the four-slot logits of the CPU test, 8 values of t: the counts equal the host function's counts for the
    same (seed, t, e) -- every draw the host function's, but for the cases below tau, which the restatement counts (at most 1 %)."""
    n = 256
    dev = _dev(n, steps=STEPS, rng_mode=1, strict=False)
    dev.reset(seeds=U.edge_seed(1, STEPS))
    dev.clone_episodes(np.zeros(n - 1, np.int32), np.arange(1, n, dtype=np.int32))
    mask = dev.action_mask
    assert (mask == mask[0]).all()
    hot = dev.get_states()
    lg, slots = U.four_slot_logits(mask[0])
    arr = np.tile(lg, (n, 1))
    counts_dev, counts_host = np.zeros((5, 4), np.int64), np.zeros((5, 4), np.int64)
    below = differ = 0
    for t in range(8):
        act, st = _sample(dev, n, arr, 3, 1, t, 1.0, 0)
        for e in range(n):
            ha = AS.from_row(hot[e], lg, 1, t, e, 1.0, False, False)[0]
            ref = AS.reference(mask[0], [False] * 5, lg, 1, t, e, 1.0, False, False, details=True)
            close = ref[3] < 2.0 ** -12 * ref[4]['zmax']
            below += int(close.sum())
            differ += int((act[e] != ha).sum())
            assert np.array_equal(act[e][~close], ha[~close]) and np.array_equal(act[e][~close], ref[0][~close]), (t, e)
            for b in range(5):
                assert act[e, b] in slots[b] and act[e, b] in (ref[0][b], ref[4]['second'][b]), (t, e, b)
                counts_dev[b, np.nonzero(slots[b] == act[e, b])[0][0]] += 1
                counts_host[b, np.nonzero(slots[b] == ha[b])[0][0]] += 1
    print('device counts', counts_dev.tolist(), 'host counts', counts_host.tolist(), 'below tau', below, 'differing draws', differ)
    assert below * 100 <= 5 * 8 * n and differ <= below
    assert np.abs(counts_dev - counts_host).sum() <= 2 * differ
    if not differ:
        assert np.array_equal(counts_dev, counts_host)
    expect = 2048 * np.array([0.4, 0.3, 0.2, 0.1])
    assert (((counts_dev - expect) ** 2 / expect).sum(axis=1) < U.chi2_bound(3)).all()
    assert _faults(dev) == 0
    dev.close()
