"""CPU: the index arithmetic of the persistent schedule (csrc/cc4_sched.h), as the kernels, the gates and the host compile it, against brute force -- the
episodes of a partition and of a policy group found by filtering range(n), a call's runs walked step by step.  The C functions come through the oracle
library (cc4o_sched_*, thin wrappers of the header); nothing here restates one of its formulas.  The shapes are the ones the GPU suite rarely visits: fewer
episodes than partitions, batches the partitions do not divide, policy groups without an episode, odd CC4_PERSIST_RUNS patterns."""
import ctypes

import numpy as np
import pytest
from oracle_binding import load

SMALL_P = (1, 2, 3, 5, 8)
BIG_P, BIG_N = 256, (1, 255, 256, 257, 5000, 6656, 8191, 8192)
SHAPES = [(P, n) for P in SMALL_P for n in range(1, 4 * P + 4)] + [(BIG_P, n) for n in BIG_N]
GROUPS = (1, 2, 3, 4)
NPH = (1, 2, 5)
RUN_PATTERNS = ((0, 1, 0, 0),       # the handle's default: CC4_PERSIST_RUNS unset
                (1, 1, 0, 0), (4, 1, 0, 0), (8, 2, 3, 1), (4, 4, 4, 4), (3, 3, 0, 7), (8, 1, 5, 0), (2, 5, 100, 0), (16, 2, 1, 1000))
I32 = ctypes.POINTER(ctypes.c_int32)
U32 = ctypes.POINTER(ctypes.c_uint32)


@pytest.fixture(scope='module')
def lib():
    return load()


def _i32(a):
    return a.ctypes.data_as(I32)


def _u32(a):
    return a.ctypes.data_as(U32)


def _limits(lib):
    out = np.zeros(7, np.uint32)
    lib.cc4o_sched_limits(_u32(out))
    return dict(zip(('step_bits', 'pg_steps', 'runner_none', 'runner_foreign', 'max_partitions', 'clear_at', 'rollout_max_k'), (int(v) for v in out)))


def _members(n, P, PG):
    """Brute force: part[p] = the episodes of partition p in rising order (range(n) dealt out to the P partitions in turn), group[p][g] = every PG-th of
    them from its number g on."""
    part = [[] for _ in range(P)]
    for e in range(n):
        part[e % P].append(e)
    group = [[part[p][g::PG] for g in range(PG)] for p in range(P)]
    return part, group


def _owner(n, PG, group):
    """... and the same the other way round: the (partition, group) counter of every episode, as one number p * PG + g."""
    owner = np.full(n, -1, np.int64)
    for p, gs in enumerate(group):
        for g, mine in enumerate(gs):
            owner[mine] = p * PG + g
    assert (owner >= 0).all()
    return owner


@pytest.mark.parametrize('P', SMALL_P + (BIG_P,))
def test_tickets_name_every_episode_run_pair_once_in_their_counters_order(lib, P):
    """Ticket coverage, ticket placement, empty counters -- with PG = 1 the counters of the balanced schedule (word 0 of every partition's line), with PG > 1
    those of a rollout."""
    for n in [s[1] for s in SHAPES if s[0] == P]:
        for PG in GROUPS:
            part, group = _members(n, P, PG)
            owner = _owner(n, PG, group)
            sizes = np.array([len(group[p][g]) for p in range(P) for g in range(PG)], np.int64)
            for nph in NPH:
                cap = n * nph + 1
                totals = np.zeros(P * PG, np.uint32)
                line, idx, j, e = (np.full(cap, -1, np.int32) for _ in range(4))
                m = lib.cc4o_sched_tickets(n, P, PG, nph, _u32(totals), _i32(line), _i32(idx), _i32(j), _i32(e), cap)
                where = f'n {n} P {P} PG {PG} nph {nph}'
                assert m == n * nph and int(totals.sum()) == m, where
                line, idx, j, e = line[:m], idx[:m], j[:m], e[:m]
                assert ((e >= 0) & (e < n)).all() and ((j >= 0) & (j < nph)).all(), where
                pairs = e.astype(np.int64) * nph + j
                assert np.unique(pairs).size == m, where                      # m distinct pairs out of the n * nph there are: every one, once
                assert (totals == sizes * nph).all(), where                   # (an empty counter hands out nothing)
                counter = np.repeat(np.arange(P * PG), totals)                # the tickets come counter by counter
                assert (line.astype(np.int64) * PG + idx == counter).all(), where
                assert (owner[e] == counter).all(), where                     # the episode is in partition `line`, in policy group `idx`
                later = np.diff(j)[np.diff(counter) == 0]                     # two neighbouring tickets of one counter:
                assert (later >= 0).all(), where                              # run-major, a counter never goes back to an earlier run


@pytest.mark.parametrize('P', SMALL_P + (BIG_P,))
def test_gate_counts_and_group_enumeration_match_the_episodes_there_are(lib, P):
    for n in [s[1] for s in SHAPES if s[0] == P]:
        # the exchange's groups of 32 neighbouring episodes
        alloc = ctypes.c_int(0)
        sizes = np.zeros(n // 32 + 8, np.int32)
        g32 = np.zeros(n, np.int32)
        groups = lib.cc4o_sched_xchg32(n, _i32(g32), _i32(sizes), ctypes.byref(alloc), sizes.size)
        blocks = [list(range(lo, min(lo + 32, n))) for lo in range(0, n, 32)]
        assert groups == len(blocks) and groups <= alloc.value <= sizes.size, n
        assert [int(v) for v in sizes[:groups]] == [len(b) for b in blocks] and int(sizes[:groups].sum()) == n, n
        assert all(int(v) <= 0 for v in sizes[groups:alloc.value]), n          # a counter row beyond the last group: the gate skips it
        assert all(int(g32[e]) == g for g, b in enumerate(blocks) for e in b), n
        for PG in GROUPS:
            where = f'n {n} P {P} PG {PG}'
            part, group = _members(n, P, PG)
            part_eps, pg_eps = np.zeros(P, np.int32), np.zeros(P * PG, np.int32)
            lib.cc4o_sched_counts(n, P, PG, _i32(part_eps), _i32(pg_eps))
            assert [max(int(v), 0) for v in part_eps] == [len(x) for x in part] and int(np.maximum(part_eps, 0).sum()) == n, where
            assert [max(int(v), 0) for v in pg_eps] == [len(group[p][g]) for p in range(P) for g in range(PG)], where
            assert int(np.maximum(pg_eps, 0).sum()) == n, where
            part_of, pgroup_of, slot = (np.zeros(n, np.int32) for _ in range(3))
            lib.cc4o_sched_episode_maps(n, P, PG, _i32(part_of), _i32(pgroup_of), _i32(slot))
            for p in range(P):
                for g in range(PG):
                    mine = group[p][g]
                    assert (part_of[mine] == p).all() and (pgroup_of[mine] == g).all(), (where, p, g)
            assert (slot == part_of * PG + pgroup_of).all(), where
            for g in range(PG):
                out = np.zeros((n // P + 1 + PG) * P, np.int32)
                threads = lib.cc4o_sched_pgroup_enum(n, P, PG, g, _i32(out), out.size)
                assert 0 <= threads <= out.size, (where, g)
                seen = out[:threads]
                assert (seen >= 0).all(), (where, g)
                seen = sorted(int(v) for v in seen if v < n)
                assert seen == sorted(e for p in range(P) for e in group[p][g]), (where, g)     # exactly group g's episodes, none twice


@pytest.mark.parametrize('pattern', RUN_PATTERNS, ids=lambda q: ','.join(map(str, q)))
def test_runs_tile_the_steps_of_a_call(lib, pattern):
    for K in list(range(1, 300)) + [500, 1000]:
        split = np.zeros(5, np.int32)
        k0, ln = np.full(K + 1, -1, np.int32), np.full(K + 1, -1, np.int32)
        nph = lib.cc4o_sched_runs(K, *pattern, 0, K + 1, _i32(split), _i32(k0), _i32(ln))
        assert 1 <= nph <= K and nph == int(split[4]) and (split >= 0).all() and split[1] + split[3] <= nph, (K, split)
        step = 0
        for r in range(nph):                                                  # walk the steps: run r starts where run r - 1 ended
            assert int(k0[r]) == step and int(ln[r]) >= 1, (K, r, split)
            step += int(ln[r])
        assert step == K, (K, split)
    K = 1 << 20
    split, k0, ln = np.zeros(5, np.int32), np.zeros(1, np.int32), np.zeros(1, np.int32)
    nph = lib.cc4o_sched_runs(K, *pattern, 0, 0, _i32(split), _i32(k0), _i32(ln))
    assert (split >= 0).all() and 1 <= nph <= K and nph == int(split[4]), split
    assert lib.cc4o_sched_runs(K, *pattern, nph - 1, 1, _i32(split), _i32(k0), _i32(ln)) == nph
    assert int(k0[0]) >= 0 and int(ln[0]) >= 1 and int(k0[0]) + int(ln[0]) == K, (split, k0, ln)


def test_default_split_known_cases(lib):
    """4 steps to a run, 8 from K = 64 on; what the runs leave over goes to single steps at the call's end."""
    split, none = np.zeros(5, np.int32), np.zeros(1, np.int32)
    for K, want in ((20, [4, 5, 1, 0, 5]), (63, [4, 15, 1, 0, 18]), (64, [8, 8, 1, 0, 8]), (500, [8, 62, 1, 0, 66])):
        lib.cc4o_sched_runs(K, 0, 1, 0, 0, 0, 0, _i32(split), _i32(none), _i32(none))
        assert split.tolist() == want, K


def test_progress_word_round_trips_and_its_limits_fit(lib):
    lim = _limits(lib)
    top = lim['clear_at'] + lim['rollout_max_k'] - 1                            # the most steps a word ever holds
    assert top <= lim['pg_steps'] == (1 << lim['step_bits']) - 1
    assert lim['runner_none'] == 0 and lim['max_partitions'] + 1 <= lim['runner_foreign'] == 511 < 1 << (32 - lim['step_bits'])
    rng = np.random.default_rng(7)
    steps = np.unique(np.concatenate([np.arange(0, 70), np.arange(top - 70, top + 1), [lim['clear_at'] - 1, lim['clear_at'], lim['clear_at'] + 1, lim['rollout_max_k']],
                                      1 << np.arange(lim['step_bits']), (1 << np.arange(1, lim['step_bits'] + 1)) - 1, rng.integers(0, top + 1, 1500)])).astype(np.uint32)
    assert int(steps.max()) == top
    s, r = (a.ravel().copy() for a in np.meshgrid(steps, np.arange(512, dtype=np.uint32), indexing='ij'))      # every runner id, 0 .. 511
    w, s2, r2 = (np.zeros(s.size, np.uint32) for _ in range(3))
    lib.cc4o_sched_progress(_u32(s), _u32(r), s.size, _u32(w), _u32(s2), _u32(r2))
    assert (s2 == s).all() and (r2 == r).all()
    assert np.unique(w).size == w.size                                          # no two (steps, runner) share a word
