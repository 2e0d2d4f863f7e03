"""GPU: the red agents as learners.  cc4_step_red_device (k_red_submit) against the host path cc4_step_ex, bit for bit, on the three step
kernels; refused records; cc4_red_view_device (k_red_view) against the host statement of the same definition (red_view.from_row) and the
independent derivation from the true-state document (red_view.from_true_state), with the leak rule, on every episode and agent; ids, snapshot
banks, faults, refusals and the ordering behind the group streams of a large batch."""
import ctypes
import json

import numpy as np
import pytest

import red_util as RU
from cage_challenge_4_amd import red_view as RV
from oracle_binding import random_actions
from view_util import DevMem, _dev, _faults, call_view

pytestmark = pytest.mark.gpu

VP = ctypes.c_void_p
ROW_H, ROW_S = 6 * 137 * 8, 6 * 16 * 4
CF_RANGE, CF_SLOT_EMPTY, CF_SLOT_CONFIG = 1, 8, 16
SHAPES = [(65, 1, '0', 'k_step_philox'), (40, 1, '1', 'k_step_philox1'), (33, 0, None, 'k_step')]
SHAPE_IDS = ['4wave', '1wave', 'numpy_stream']


def _docs(dev):
    return RU.parse([dev.true_state_json(e) for e in range(dev.num_envs)])


class RedStepper:
    """The device path of one handle: blue indices and red words uploaded into device memory of the test's, then cc4_step_red_device (or, red
    None, cc4_step_device) and a fetch."""

    def __init__(self, dev):
        self.dev, n = dev, dev.num_envs
        self.d_act, self.d_red = DevMem(n * 5 * 4), DevMem(n * 6 * 4 * 4)

    def step(self, actions, words):
        dev = self.dev
        self.d_act.up(np.ascontiguousarray(actions, np.int32))
        if words is None:
            dev._chk(dev.lib.cc4_step_device(dev._h, self.d_act.p, None), 'cc4_step_device')
        else:
            self.d_red.up(np.ascontiguousarray(words, np.int32))
            dev.step_red_device(self.d_act.p, None, self.d_red.p)
        obs, rew, done = dev._fetch()
        return obs.copy(), rew.copy(), done.copy(), dev.err.copy()

    def free(self):
        self.d_act.free(); self.d_red.free()


def _same_outputs(a, b, what):
    for x, y, name in zip(a, b, ('obs', 'reward', 'done', 'err')):
        assert np.array_equal(x, y), (what, name, np.argwhere(np.asarray(x) != np.asarray(y))[:6].tolist())


def _same_episodes(A, B, what):
    sa, sb = A.get_states(), B.get_states()
    assert np.array_equal(sa, sb), (what, 'hot rows', sorted(set(np.argwhere(sa != sb)[:, 0].tolist()))[:8])
    for e in range(A.num_envs):          # the cold rows on their live extents: everything the document reports from them
        assert A.true_state_json(e) == B.true_state_json(e), (what, 'true state', e)
    assert np.array_equal(A.rng_state(), B.rng_state()), (what, 'generator positions')


@pytest.mark.parametrize('n,rng_mode,lean,kernel', SHAPES, ids=SHAPE_IDS)
def test_device_submission_equals_the_host_path(monkeypatch, n, rng_mode, lean, kernel):
    """Two handles, 40 steps: A takes the records through cc4_step_ex (SID_AUTO resolved on the host), B the same words through
    cc4_step_red_device.  Outputs after every step; rows, true-state documents and generator positions at the end.  The run must have resolved
    every red action type 0..8 at least once."""
    if lean is not None:
        monkeypatch.setenv('CC4_PHILOX_LEAN', lean)
    seed, T = 7100 + n, 40
    A = _dev(n, steps=60, rng_mode=rng_mode, autoreset=True, strict=False)
    B = _dev(n, steps=60, rng_mode=rng_mode, autoreset=True, strict=False)
    assert A.step_kernel == kernel and B.step_kernel == kernel
    A.reset(seeds=seed); B.reset(seeds=seed)
    stepper, rng = RedStepper(B), np.random.default_rng(seed)
    resolved, autos, explicit = set(), 0, 0
    docs = _docs(A)
    for t in range(T):
        words = RU.red_words(docs, rng)
        live = words[..., 0] != -1
        autos += int((words[..., 3][live] == RV.SID_AUTO).sum()); explicit += int((words[..., 3][live] != RV.SID_AUTO).sum())
        blue = random_actions(seed, t, n)
        oa, ra, da, _ = A.step_ex(blue, None, red=RU.host_records(words, docs))
        _same_outputs((oa, ra, da, A.err), stepper.step(blue, words), t)
        docs = _docs(A)
        resolved |= RU.resolved_types(docs)
    _same_episodes(A, B, 'after the last step')
    assert set(range(9)) <= resolved, sorted(resolved)
    assert autos > 100 and explicit > 100, (autos, explicit)
    assert _faults(B) == 0
    stepper.free(); A.close(); B.close()


def test_refused_records_become_none_and_stale_records_are_cleared():
    n, seed = 24, 612
    A = _dev(n, steps=60, rng_mode=1, strict=False)
    B = _dev(n, steps=60, rng_mode=1, strict=False)
    A.reset(seeds=seed); B.reset(seeds=seed)
    stepper, rng = RedStepper(B), np.random.default_rng(seed)
    docs = _docs(A)
    for t in range(6):                    # a few steps with red actions first: sessions, queued actions
        words = RU.red_words(docs, rng)
        blue = random_actions(seed, t, n)
        A.step_ex(blue, None, red=RU.host_records(words, docs))
        stepper.step(blue, words)
        docs = _docs(A)
    assert _faults(B) == 0
    words = RU.red_words(docs, rng, p_none=0.0)
    bad = {(3, 0): (11, 5, 0, 0), (7, 0): (4, 137, 0, RV.SID_AUTO), (11, 2): (0, 0, 9, RV.SID_AUTO), (20, 5): (8, 3, 200, 1)}
    for (e, r), w in bad.items():
        words[e, r] = w
    clean = words.copy()
    for (e, r) in bad:
        clean[e, r] = (-1, 0, 0, 0)
    blue = random_actions(seed, 6, n)
    oa, ra, da, _ = A.step_ex(blue, None, red=RU.host_records(clean, docs))
    _same_outputs((oa, ra, da, A.err), stepper.step(blue, words), 'refused records')
    assert _faults(B) == CF_RANGE and _faults(B) == 0
    _same_episodes(A, B, 'after the step with refused records')
    # a plain device step next: the records of the last call must not act again
    none = A.agent_actions('red')
    blue = random_actions(seed, 7, n)
    oa, ra, da, _ = A.step_ex(blue, None, red=none)
    _same_outputs((oa, ra, da, A.err), stepper.step(blue, None), 'plain step after red actions')
    _same_episodes(A, B, 'after the plain step')
    # refusals of the call itself: -2, nothing enqueued
    lib, h = B.lib, B._h
    assert lib.cc4_step_red_device(h, stepper.d_act.p, None, None) == -2 and b'cc4_step_device' in lib.cc4_last_error(h)
    assert lib.cc4_step_red_device(h, stepper.d_act.p, None, stepper.d_red.at(4)) == -2 and b'aligned' in lib.cc4_last_error(h)
    _same_episodes(A, B, 'after the refused calls')
    assert _faults(B) == 0
    stepper.free(); A.close(); B.close()


def test_green_records_are_none_whatever_came_before():
    """The record buffer exists before any record was written when a handle's first cc4_step_ex is refused; and it holds green records after a
    cc4_step_ex with green actions.  In both cases a following cc4_step_red_device must leave every green record none: the episodes equal those
    of a handle that takes the same red records through cc4_step_ex with no green entry."""
    n, seed = 24, 733
    A = _dev(n, steps=60, rng_mode=1, strict=False)
    B = _dev(n, steps=60, rng_mode=1, strict=False)
    A.reset(seeds=seed); B.reset(seeds=seed)
    stepper, rng = RedStepper(B), np.random.default_rng(seed)
    bad = B.agent_actions('red')
    bad['type'][5, 1], bad['host'][5, 1] = 4, 200                     # a host past the table: refused, nothing stepped
    with pytest.raises(Exception, match='out of range'):
        B.step_ex(random_actions(seed, 0, n), None, red=bad)
    _same_episodes(A, B, 'after the refused cc4_step_ex')
    docs = _docs(A)
    for t in range(3):
        words = RU.red_words(docs, rng)
        blue = random_actions(seed, t, n)
        oa, ra, da, _ = A.step_ex(blue, None, red=RU.host_records(words, docs))
        _same_outputs((oa, ra, da, A.err), stepper.step(blue, words), ('after a refused cc4_step_ex', t))
        docs = _docs(A)
    _same_episodes(A, B, 'red device steps after a refused cc4_step_ex')
    # green actions through cc4_step_ex on both, then red actions alone: the green records of that step must not act again
    green = A.agent_actions('green')
    for e, d in enumerate(docs):
        for g in range(d['n_green']):
            green['type'][e, g], green['host'][e, g] = g % 3, d['green_hosts'][g]
    blue = random_actions(seed, 3, n)
    oa, ra, da, _ = A.step_ex(blue, None, green=green)
    ob, rb, db, _ = B.step_ex(blue, None, green=green)
    _same_outputs((oa, ra, da, A.err), (ob, rb, db, B.err), 'green step')
    docs = _docs(A)
    for t in range(4, 7):
        words = RU.red_words(docs, rng)
        blue = random_actions(seed, t, n)
        oa, ra, da, _ = A.step_ex(blue, None, red=RU.host_records(words, docs))
        _same_outputs((oa, ra, da, A.err), stepper.step(blue, words), ('after green actions', t))
        docs = _docs(A)
    _same_episodes(A, B, 'red device steps after green actions')
    assert _faults(B) == 0
    stepper.free(); A.close(); B.close()


def _view(dev, n, ids=None, bank=None, cap=0, fill=0):
    """cc4_red_view_device into a fresh device buffer [hosts | scalars], then synchronise and copy down."""
    def call(d_bank, cap, d_ids, n, p_hosts, p_scal):
        dev.red_view_device(p_hosts, p_scal, n=n, d_ids=d_ids, d_bank=d_bank, capacity=cap)
    return call_view(dev, call, n, ((np.uint8, (6, 137, 8)), (np.int32, (6, 16))), ids, bank, cap, fill)


def _from_rows(rows):
    hs = [RV.from_row(r) for r in rows]
    return np.stack([h for h, _ in hs]), np.stack([s for _, s in hs])


@pytest.mark.parametrize('n,rng_mode,lean,kernel', SHAPES, ids=SHAPE_IDS)
def test_view_kernel_equals_host_function_equals_the_document(monkeypatch, n, rng_mode, lean, kernel):
    """All four scripted red classes in one batch (cc4_set_policies), 36 steps of random blue actions; at four checkpoints, for EVERY episode
    and agent: kernel == from_row on all columns, == from_true_state on the columns the document defines, the leak rule for every host, and
    busy == 0 -> queued type 11.  The run must show a root session, an abstract session, an inactive and a busy agent."""
    if lean is not None:
        monkeypatch.setenv('CC4_PHILOX_LEAN', lean)
    seed, T = 5200 + n, 36
    dev = _dev(n, steps=80, rng_mode=rng_mode, strict=False)
    assert dev.step_kernel == kernel
    dev.set_policies(red=(np.arange(n) % 4).astype(np.int8))
    dev.reset(seeds=seed)
    assert sorted(set(dev.policies()[0][:, 0].tolist())) == [0, 1, 2, 3]
    seen = dict(root=0, abstract=0, inactive=0, busy=0, obs=0)
    doc_words = list(RV.DOC_WORDS)

    def check(what):
        hosts, scal = dev.red_view()
        assert hosts.shape == (n, 6, 137, 8) and hosts.dtype == np.uint8 and scal.shape == (n, 6, 16) and scal.dtype == np.int32
        want_h, want_s = _from_rows(dev.get_states())
        bad = np.argwhere(hosts != want_h)
        assert bad.size == 0, (what, [tuple(map(int, b)) + (int(hosts[tuple(b)]), int(want_h[tuple(b)])) for b in bad[:8]])
        assert np.array_equal(scal, want_s), (what, np.argwhere(scal != want_s)[:8].tolist())
        for e, d in enumerate(_docs(dev)):
            th, ts = RV.from_true_state(d)
            assert np.array_equal(hosts[e], th), (what, e, np.argwhere(hosts[e] != th)[:8].tolist())
            assert np.array_equal(scal[e][:, doc_words], ts[:, doc_words]), (what, e, scal[e].tolist(), ts.tolist())
            assert not hosts[e][~RU.allowed_rows(d)].any(), (what, e, 'a row of a host the agent knows nothing of is not zero')
        assert (scal[..., 2][scal[..., 1] == 0] == 11).all() and (scal[..., 3][scal[..., 1] == 0] == 255).all() and (scal[..., 4][scal[..., 1] == 0] == 0).all()
        assert (hosts[..., 7] == 0).all()
        seen['root'] += int((hosts[..., 2] == 2).any(axis=2).sum()); seen['abstract'] += int((hosts[..., 5] == 1).any(axis=2).sum())
        seen['inactive'] += int((scal[..., 0] == 0).sum()); seen['busy'] += int((scal[..., 1] == 1).sum()); seen['obs'] += int((hosts[..., 4] != 0).sum())
        return hosts, scal

    check('reset')
    for t in range(T):
        dev.step(random_actions(seed, t, n))
        if t + 1 in (1, 17, T):
            _h, scal = check(t + 1)
            assert (scal[..., 15] == t + 1).all()
    assert all(v > 0 for v in seen.values()), seen
    dev.close()


def test_view_ids_banks_faults_and_refusals():
    n, steps = 48, 30
    dev = _dev(n, steps=steps, rng_mode=1, strict=False)
    dev.reset(seeds=88)
    for t in range(12):
        dev.step(random_actions(88, t, n))
    lib, h = dev.lib, dev._h
    all_h, all_s = dev.red_view()
    want = _from_rows(dev.get_states())
    assert np.array_equal(all_h, want[0]) and np.array_equal(all_s, want[1]) and (all_s[..., 15] == 12).all()
    # a shuffled id list with duplicates: rows in the order asked for
    rng = np.random.default_rng(3)
    ids = np.concatenate([rng.permutation(n)[:20], [5, 5, 47, 0, 5]]).astype(np.int32)
    hosts, scal = _view(dev, len(ids), ids=ids)
    assert np.array_equal(hosts, all_h[ids]) and np.array_equal(scal, all_s[ids])
    hosts, scal = dev.red_view(ids[:7])
    assert np.array_equal(hosts, all_h[ids[:7]]) and np.array_equal(scal, all_s[ids[:7]])
    # n = 0: a no-op
    canary = DevMem(ROW_H + ROW_S, 0xC3)
    assert lib.cc4_red_view_device(h, None, 0, None, 0, canary.p, canary.at(ROW_H)) == 0
    dev.synchronize()
    assert (canary.down(np.uint8, canary.nbytes) == 0xC3).all()
    assert dev.red_view(np.zeros(0, np.int32))[0].shape == (0, 6, 137, 8)

    # 16 episodes into a bank; the env steps on; the bank's slots still show the view at the save
    slot, cap = int(lib.cc4_snapshot_bytes(h)), 20
    bank = DevMem(cap * slot)
    src = np.arange(3, 3 + 16, dtype=np.int32)
    dst = rng.permutation(16).astype(np.int32)
    idx = DevMem(4 * 32)
    idx.up(src); idx.up(dst, 64)
    assert lib.cc4_copy_episodes_device(h, 16, None, 0, idx.p, bank.p, cap, idx.at(64), None) == 0, lib.cc4_last_error(h)
    for t in range(12, 15):
        dev.step(random_actions(88, t, n))
    now_h, now_s = dev.red_view()
    assert (now_s[..., 15] == 15).all() and not np.array_equal(now_s[src], all_s[src])
    hosts, scal = _view(dev, 16, ids=dst, bank=bank, cap=cap)
    assert np.array_equal(hosts, all_h[src]) and np.array_equal(scal, all_s[src])
    inv = np.argsort(dst)
    hosts, scal = _view(dev, 16, bank=bank, cap=cap)                 # no id list: slots 0 .. 15
    assert np.array_equal(hosts, all_h[src[inv]]) and np.array_equal(scal, all_s[src[inv]])
    assert _faults(dev) == 0

    # a slot written by a handle of another episode length: its header and the head of its row into slot 18
    other = _dev(2, steps=steps + 10, rng_mode=1)
    other.reset(seeds=9)
    oslot = int(other.lib.cc4_snapshot_bytes(other._h))
    obank = DevMem(oslot)
    zero = DevMem(16)
    assert other.lib.cc4_copy_episodes_device(other._h, 1, None, 0, zero.p, obank.p, 1, zero.p, None) == 0
    other.synchronize()
    bank.up(obank.down(np.uint8, min(slot, oslot)), 18 * slot)
    other.close()
    by_slot = {int(d): int(s) for s, d in zip(src, dst)}
    for bad_id, bit in ((17, CF_SLOT_EMPTY), (cap, CF_RANGE), (-1, CF_RANGE), (18, CF_SLOT_CONFIG)):
        hosts, scal = _view(dev, 3, ids=[2, bad_id, 9], bank=bank, cap=cap, fill=0x77)
        assert not hosts[1].any() and not scal[1].any(), bad_id
        assert np.array_equal(hosts[0], all_h[by_slot[2]]) and np.array_equal(hosts[2], all_h[by_slot[9]]) and np.array_equal(scal[2], all_s[by_slot[9]])
        assert _faults(dev) == bit, (bad_id, bit)
    hosts, scal = _view(dev, 4, ids=[n, 1, -5, 46], fill=0x77)          # the handle's own episodes: ids past the batch
    assert not hosts[0].any() and not hosts[2].any() and not scal[0].any() and not scal[2].any()
    assert np.array_equal(hosts[1], now_h[1]) and np.array_equal(hosts[3], now_h[46]) and np.array_equal(scal[3], now_s[46])
    assert _faults(dev) == CF_RANGE and _faults(dev) == 0
    with pytest.raises(Exception, match='INDEX_OUT_OF_RANGE'):
        dev.red_view([0, n])

    # refusals: -2, nothing enqueued, the output untouched
    out = DevMem(2 * (ROW_H + ROW_S), 0xC3)
    assert lib.cc4_red_view_device(h, None, 0, None, -1, out.p, out.at(2 * ROW_H)) == -2
    assert lib.cc4_red_view_device(h, None, 0, None, 2, None, out.at(2 * ROW_H)) == -2
    assert lib.cc4_red_view_device(h, None, 0, None, 2, out.at(8), out.at(2 * ROW_H)) == -2 and b'aligned' in lib.cc4_last_error(h)
    assert lib.cc4_red_view_device(h, bank.p, 0, None, 2, out.p, out.at(2 * ROW_H)) == -2 and b'capacity' in lib.cc4_last_error(h)
    assert lib.cc4_red_view_device(h, bank.p, -3, None, 2, out.p, out.at(2 * ROW_H)) == -2
    dev.synchronize()
    assert (out.down(np.uint8, out.nbytes) == 0xC3).all() and _faults(dev) == 0
    assert lib.cc4_red_view_device(h, None, 0, None, 2, out.p, None) == 0            # the agent words are optional
    dev.synchronize()
    assert np.array_equal(out.down(np.uint8, (2, 6, 137, 8)), now_h[:2]) and (out.down(np.uint8, 2 * ROW_S, 2 * ROW_H) == 0xC3).all()
    for m in (canary, bank, idx, obank, zero, out):
        m.free()
    dev.close()


def test_calls_are_ordered_behind_the_group_streams_of_a_large_batch():
    """6656 counter-mode episodes: a step is several launches on several streams.  run_random_steps(12), two cc4_step_device, a
    cc4_step_red_device whose SID_AUTO reads the rows those steps leave, then the view, with no synchronise in between -- against a second handle
    that takes the same steps one synchronised call at a time."""
    n, steps, seed0 = 6656, 200, 515
    dev = _dev(n, steps=steps, rng_mode=1, autoreset=True, strict=False)
    ref = _dev(n, steps=steps, rng_mode=1, autoreset=True, strict=False)
    assert dev.launches_per_step > 1 and dev.step_kernel == 'k_step_philox1'
    dev.reset(seeds=seed0); ref.reset(seeds=seed0)
    words = np.zeros((n, 6, 4), np.int32)
    words[..., 0] = -1
    words[:, 0, 0], words[:, 0, 2], words[:, 0, 3] = 0, np.arange(n) % 9, RV.SID_AUTO         # red_agent_0: DiscoverRemoteSystems on its first session
    buf, d_red = DevMem(n * (ROW_H + ROW_S), 0xEE), DevMem(words.nbytes)
    d_red.up(words)
    acts = VP()
    dev._chk(dev.lib.cc4_actions_device(dev._h, ctypes.byref(acts)), 'cc4_actions_device')
    lib, h = dev.lib, dev._h
    dev.run_random_steps(seed0, 0, 12, timed=False)
    rc = lib.cc4_step_device(h, acts, None) or lib.cc4_step_device(h, acts, None)
    rc = rc or lib.cc4_step_red_device(h, acts, None, d_red.p)
    rc = rc or lib.cc4_red_view_device(h, None, 0, None, n, buf.p, buf.at(n * ROW_H))
    assert rc == 0, lib.cc4_last_error(h)
    dev.synchronize()
    hosts, scal = buf.down(np.uint8, (n, 6, 137, 8)), buf.down(np.int32, (n, 6, 16), n * ROW_H)
    rows = dev.get_states()
    want_h, want_s = _from_rows(rows[::13])
    assert (want_s[..., 15] == 15).all()
    assert np.array_equal(hosts[::13], want_h) and np.array_equal(scal[::13], want_s)
    # the reference handle: the same fifteen steps, every call synchronised
    ref.run_random_steps(seed0, 0, 12, timed=False)
    last = ref.device_actions().copy()
    ref.step(last); ref.step(last)
    docs = {e: json.loads(ref.true_state_json(e)) for e in range(0, n, 97)}
    rec = ref.agent_actions('red')
    rec['type'][:, 0], rec['arg'][:, 0] = 0, np.arange(n) % 9
    st = ref.get_states()
    for e in range(n):
        sid = int(RV.from_row(st[e])[1][0, 12])                      # SID_AUTO on the host: the first listed session, 0 if none
        rec['session'][e, 0] = 0 if sid == RV.SID_NONE else sid
    for e, d in docs.items():
        assert rec['session'][e, 0] == RV.auto_sid(d, 0)
    ref.step_ex(last, None, red=rec)
    bad = sorted(set(np.argwhere(rows != ref.get_states())[:, 0].tolist()))
    assert not bad, (len(bad), bad[:10])
    assert _faults(dev) == 0
    buf.free(); d_red.free()
    dev.close(); ref.close()


def test_refused_while_a_rollout_is_in_flight():
    n, K = 8192, 4
    dev = _dev(n, steps=50, rng_mode=1)
    dev.reset(seeds=4)
    lib, h = dev.lib, dev._h
    out = DevMem(2 * (ROW_H + ROW_S), 0xC3)
    d_red = DevMem(n * 6 * 4 * 4, 0xFF)
    acts = VP()
    dev._chk(lib.cc4_actions_device(h, ctypes.byref(acts)), 'cc4_actions_device')
    assert lib.cc4_rollout_begin(h, K) == 0, lib.cc4_last_error(h)
    assert lib.cc4_red_view_device(h, None, 0, None, 2, out.p, out.at(2 * ROW_H)) == -2 and b'rollout' in lib.cc4_last_error(h)
    assert lib.cc4_step_red_device(h, acts, None, d_red.p) == -2 and b'rollout' in lib.cc4_last_error(h)
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
    assert dev.run_kernel_for(12) == 'k_run_philox1'                         # the refused call left the handle on its one-launch forms
    assert lib.cc4_red_view_device(h, None, 0, None, 2, out.p, out.at(2 * ROW_H)) == 0          # after the rollout: fine
    dev.synchronize()
    want_h, want_s = _from_rows([dev.get_state(0), dev.get_state(1)])
    assert np.array_equal(out.down(np.uint8, (2, 6, 137, 8)), want_h) and np.array_equal(out.down(np.int32, (2, 6, 16), 2 * ROW_H), want_s)
    assert (want_s[..., 15] == K).all()
    out.free(); d_red.free()
    dev.close()
