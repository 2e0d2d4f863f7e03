"""GPU: the one row resolver of the derived views (view_rows, csrc/cc4_view_src.h), tested once for all five of them -- k_state_features,
k_red_view, k_blue_view, k_blue_edges, k_reward_terms.  Entry i reads episode ids[i] of the handle, or the rows inside slot ids[i] of a snapshot
bank; an index out of range, a slot never written and a slot of another configuration each give the view's empty output in that entry alone and
exactly their bit in the handle's fault word.  These are refused entries reported through a flag word: nothing here faults the GPU."""
import numpy as np
import pytest

from cage_challenge_4_amd import blue_edges as BE
from cage_challenge_4_amd import blue_view as BV
from cage_challenge_4_amd import red_view as RV
from cage_challenge_4_amd import reward_terms as RT
from cage_challenge_4_amd import state_features as SF
from oracle_binding import random_actions
from view_util import DevMem, _dev, _faults, call_view

pytestmark = pytest.mark.gpu

N, STEPS, CAP, E = 16, 30, 6, 48
CF_RANGE, CF_SLOT_EMPTY, CF_SLOT_CONFIG = 1, 8, 16
SAVED = (5, 9, 12)                     # the episodes in slots 0, 1, 2
# bank slot -> the bit it raises: 3 was never written, 4 holds the head of a slot of a handle with STEPS + 10, 6 and -1 are no slots
BAD = ((3, CF_SLOT_EMPTY), (4, CF_SLOT_CONFIG), (CAP, CF_RANGE), (-1, CF_RANGE))
# view -> entry point, arguments in front of the outputs, (dtype, shape of one entry, the empty output's fill) of the two outputs, from_row of
# (hot row, cold row)
VIEWS = {
    'state_features': ('cc4_state_features_device', (), ((np.uint8, (137, 16), 0), (np.int32, (32,), 0)), lambda hot, cold: SF.from_row(hot)),
    'red_view': ('cc4_red_view_device', (), ((np.uint8, (6, 137, 8), 0), (np.int32, (6, 16), 0)), lambda hot, cold: RV.from_row(hot)),
    'blue_view': ('cc4_blue_view_device', (), ((np.uint8, (5, 137, 8), 0), (np.int32, (5, 16), 0)), lambda hot, cold: BV.from_row(hot, cold, STEPS)),
    'blue_edges': ('cc4_blue_edges_device', (E,), ((np.int32, (E, 8), -1), (np.int32, (8,), 0)), lambda hot, cold: BE.from_row(hot, cold, STEPS, E)),
    'reward_terms': ('cc4_reward_terms_device', (), ((np.int32, (9, 4), 0), (np.int32, (16,), 0)), lambda hot, cold: RT.from_row(hot, cold, STEPS)),
}


@pytest.fixture(scope='module')
def world():
    """One handle of 16 counter-mode episodes of 30 steps, event log and reward terms on, five steps in; a bank of six slots (SAVED, BAD); the
    rows of every episode as they were at the save and, one step later, as they are now."""
    dev = _dev(N, steps=STEPS, rng_mode=1, strict=False)
    dev.reset(seeds=61)
    dev.enable_event_log(True)
    dev.enable_reward_terms()
    for t in range(5):
        dev.step(random_actions(61, t, N))
    lib, h = dev.lib, dev._h
    rows = lambda: [(dev.get_state(e), dev.get_cold(e)) for e in range(N)]      # noqa: E731
    at_save = rows()
    slot = int(lib.cc4_snapshot_bytes(h))
    bank, idx = DevMem(CAP * slot), DevMem(128)
    idx.up(np.asarray(SAVED, np.int32)); idx.up(np.arange(len(SAVED), dtype=np.int32), 64)
    assert lib.cc4_copy_episodes_device(h, len(SAVED), None, 0, idx.p, bank.p, CAP, idx.at(64), None) == 0, lib.cc4_last_error(h)
    dev.step(random_actions(61, 5, N))                 # the handle moves on: a slot shows the episode as it was saved
    now = rows()
    assert not np.array_equal(now[SAVED[1]][0], at_save[SAVED[1]][0])
    # a slot written by a handle of another episode length: its header and the head of its rows into slot 4
    other = _dev(2, steps=STEPS + 10, rng_mode=1)
    other.reset(seeds=9)
    oslot = int(other.lib.cc4_snapshot_bytes(other._h))
    obank, zero = DevMem(oslot), DevMem(16)
    assert other.lib.cc4_copy_episodes_device(other._h, 1, None, 0, zero.p, obank.p, 1, zero.p, None) == 0
    other.synchronize()
    bank.up(obank.down(np.uint8, min(slot, oslot)), 4 * slot)
    other.close()
    assert _faults(dev) == 0
    yield dev, bank, at_save, now
    for m in (bank, idx, obank, zero):
        m.free()
    dev.close()


@pytest.mark.parametrize('view', list(VIEWS))
def test_every_view_resolves_its_entries_alike(world, view):
    dev, bank, at_save, now = world
    entry, extra, outs, from_row = VIEWS[view]
    parts = [(dt, shape) for dt, shape, _fill in outs]
    empty = [np.full(shape, fill, dt) for dt, shape, fill in outs]

    def call(d_bank, cap, d_ids, n, p0, p1):
        assert getattr(dev.lib, entry)(dev._h, d_bank, cap, d_ids, n, *extra, p0, p1) == 0, dev.lib.cc4_last_error(dev._h)

    def check(got, i, want, what):
        for k in (0, 1):
            assert got[k][i].dtype == want[k].dtype and got[k][i].tobytes() == want[k].tobytes(), (view, what, 'entry', i, 'output', k)

    saved = [from_row(*at_save[e]) for e in SAVED]     # what slots 0, 1, 2 show
    # each bad slot alone between two good ones
    for bad, bit in BAD:
        got = call_view(dev, call, 3, parts, ids=[1, bad, 2], bank=bank, cap=CAP, fill=0x77)
        check(got, 0, saved[1], bad); check(got, 1, empty, bad); check(got, 2, saved[2], bad)
        assert _faults(dev) == bit, (view, bad)
        assert _faults(dev) == 0
    # all of them in one call: the OR of their bits, the good entries untouched
    ids = [1] + [bad for bad, _bit in BAD] + [2, 0]
    got = call_view(dev, call, len(ids), parts, ids=ids, bank=bank, cap=CAP, fill=0x77)
    check(got, 0, saved[1], 'all'); check(got, len(ids) - 2, saved[2], 'all'); check(got, len(ids) - 1, saved[0], 'all')
    for i in range(1, 1 + len(BAD)):
        check(got, i, empty, 'all')
    assert _faults(dev) == CF_RANGE | CF_SLOT_EMPTY | CF_SLOT_CONFIG
    assert _faults(dev) == 0
    # the handle's own episodes: indices past the batch on either side
    got = call_view(dev, call, 3, parts, ids=[N, 1, -1], fill=0x77)
    check(got, 0, empty, 'own'); check(got, 1, from_row(*now[1]), 'own'); check(got, 2, empty, 'own')
    assert _faults(dev) == CF_RANGE
    assert _faults(dev) == 0
