"""CPU: the self-check's digest (CC4_PERSIST_VERIFY; the definition: csrc/cc4_digest.h, shared by k_digest and cc4_debug_digest_rows; the prose:
include/cc4_debug.h) -- the instrument every `verify_stats() == (calls, 0)` of the GPU suite reads.  Every comparison is exact.

* The numpy restatement of the prose (tests/digest_util.py) against the host function, on rows the oracle produced and on random bytes.
* Sensitivity, exhaustive over the 16-byte vectors of a hot and a cold row: a bit flipped in any of them moves its word and no other, and no two flips
  give the same word -- a vector loop that stops short, a lane that is skipped, a sum that cancels would show here.
* Sensitivity of the outputs word to every observation value, each action, reward, done and the error word.
* Order: vectors exchanged within a lane's chain, across lanes of one round, observation values exchanged within a lane.
tests/test_self_check_fires.py holds the kernel against both and shows a checked call reporting a planted difference."""
import ctypes

import numpy as np
import pytest

import digest_util as D
from oracle_binding import OracleVecEnv, random_actions

N = 3


def _episodes(rng_mode, steps, after):
    """(hot, cold, obs, reward, done, err, actions) of N oracle episodes after `after` steps of the stand-in policy's draws."""
    ora = OracleVecEnv(N, steps=steps, rng_mode=rng_mode, autoreset=True)
    ora.reset_batch(31 + rng_mode)
    a = np.zeros((N, 5), np.int32)
    for t in range(after):
        a = random_actions(31, t, N)
        ora.step_batch(a)
    out = [(ora.get_state(i), ora.get_cold(i), ora._obs[i].copy(), float(ora._rew[i]), int(ora._done[i]), int(ora._err[i]), a[i].copy()) for i in range(N)]
    ora.close()
    return out


@pytest.fixture(scope='module')
def base():
    """One 40-step episode after 25 steps (numpy stream): the row the sensitivity tests flip bits of.  Nobody writes to it."""
    ep = _episodes(0, 40, 25)[1]
    for a in ep:
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return ep


def _random_episode(rng, cold_bytes):
    from cage_challenge_4_amd import _lib
    hot = rng.integers(0, 256, int(_lib.load().cc4_state_bytes()), dtype=np.uint8)
    cold = rng.integers(0, 256, cold_bytes, dtype=np.uint8)
    obs = rng.integers(-2**31, 2**31, D.OBS, dtype=np.int64).astype(np.int32)
    act = rng.integers(-2**31, 2**31, D.NBLUE, dtype=np.int64).astype(np.int32)
    return hot, cold, obs, float(np.float32(rng.normal() * 1e3)), int(rng.integers(0, 256)), int(rng.integers(0, 2**32)), act


@pytest.mark.parametrize('steps', [40, 500])
@pytest.mark.parametrize('rng_mode', [0, 1], ids=['numpy-stream', 'counter'])
def test_restatement_equals_host_function_on_oracle_rows(rng_mode, steps):
    sizes = set()
    for after in (0, 1, 25):
        for i, ep in enumerate(_episodes(rng_mode, steps, after)):
            want, got = D.digest(*ep), D.host_digest(*ep)
            assert np.array_equal(want, got), (rng_mode, steps, after, i, [hex(int(v)) for v in want], [hex(int(v)) for v in got])
            sizes.add(ep[1].size)
    assert len(sizes) == 1 and sizes.pop() % 16 == 0


def test_the_two_episode_lengths_give_two_cold_row_sizes():
    assert _episodes(0, 40, 0)[0][1].size < _episodes(0, 500, 0)[0][1].size


def test_restatement_equals_host_function_on_random_bytes():
    rng = np.random.default_rng(20)
    for cold_bytes in (16, 16 * 63, 16 * 64, 16 * 65, 16 * 129, 16 * 5000 + 16):      # fewer vectors than lanes, a full round, one more, an odd count
        for _ in range(3):
            ep = _random_episode(rng, cold_bytes)
            assert np.array_equal(D.digest(*ep), D.host_digest(*ep)), cold_bytes
    # extreme values of every output
    hot, cold, obs, _, _, _, act = _random_episode(rng, 64)
    for reward, done, err in ((0.0, 0, 0), (-0.0, 1, 0xFFFFFFFF), (np.float32(3.4e38), 255, 1 << 31), (-1.5, 1, 1 << 7)):
        ep = (hot, cold, obs, float(reward), done, err, act)
        assert np.array_equal(D.digest(*ep), D.host_digest(*ep)), (reward, done, err)


def test_host_function_refuses_bad_arguments(base):
    from cage_challenge_4_amd import _lib
    lib, vp = _lib.load(), ctypes.c_void_p
    hot, cold, obs, reward, done, err, act = [np.array(a) if isinstance(a, np.ndarray) else a for a in base]
    out = np.full(3, 7, np.uint64)
    P = lambda a: a.ctypes.data_as(vp)          # noqa: E731
    assert lib.cc4_debug_digest_rows(P(hot), P(cold), cold.size - 8, P(obs), reward, done, err, P(act), P(out)) == -2
    assert lib.cc4_debug_digest_rows(None, P(cold), cold.size, P(obs), reward, done, err, P(act), P(out)) == -2
    assert lib.cc4_debug_digest_rows(P(hot), P(cold), cold.size, P(obs), reward, done, err, P(act), None) == -2
    assert (out == 7).all()


def _flips(row):
    """Per 16-byte vector index: the row with bit 0 of the vector's first byte flipped, and with bit 7 of its last byte flipped."""
    for v in range(row.size // 16):
        for byte, bit in ((16 * v, 1), (16 * v + 15, 0x80)):
            r = row.copy()
            r[byte] ^= bit
            yield v, byte, r


@pytest.mark.parametrize('which', [0, 1], ids=['hot', 'cold'])
def test_every_vector_of_a_row_moves_its_word_and_no_other(base, which):
    ep = list(base)
    clean = D.host_digest(*ep)
    row = np.array(ep[which])
    assert row.size % 16 == 0 and row.size // 16 > 2 * D.LANES         # every lane, more than one round
    words = []
    for v, byte, r in _flips(row):
        ep[which] = r
        got = D.host_digest(*ep)
        other = [i for i in range(3) if i != which]
        assert got[which] != clean[which], (which, v, byte)
        assert np.array_equal(got[other], clean[other]), (which, v, byte)
        words.append(int(got[which]))
        if v % 97 == 0 or v >= row.size // 16 - 2:                     # the restatement follows, first and last vectors included
            assert int(D.row_word(r)) == int(got[which]), (which, v, byte)
    assert len(words) == 2 * (row.size // 16) and len(set(words)) == len(words), (which, len(words), len(set(words)))


def test_every_output_moves_the_outputs_word_and_no_other(base):
    hot, cold, obs, reward, done, err, act = base
    clean = D.host_digest(*base)
    words = []

    def check(what, *ep):
        got = D.host_digest(hot, cold, *ep)
        assert got[2] != clean[2], what
        assert np.array_equal(got[:2], clean[:2]), what
        assert np.array_equal(D.digest(hot, cold, *ep), got), what
        words.append(int(got[2]))
    for i in range(D.OBS):
        for bit in (1, -2**31):                    # bit 0 and bit 31 of the value
            o = np.array(obs)
            o[i] ^= np.int32(bit)
            check(('obs', i, bit), o, reward, done, err, act)
    for b in range(D.NBLUE):
        for bit in (1, -2**31):
            a = np.array(act)
            a[b] ^= np.int32(bit)
            check(('action', b, bit), obs, reward, done, err, a)
    for bits in (1, 1 << 31):
        r = float((np.array([reward], np.float32).view(np.uint32) ^ np.uint32(bits)).view(np.float32)[0])
        check(('reward', bits), obs, r, done, err, act)
    for d in (done ^ 1, done ^ 0x80):
        check(('done', d), obs, reward, d, err, act)
    for bits in (1, 1 << 31):
        check(('err', bits), obs, reward, done, err ^ bits, act)
    assert len(set(words)) == len(words) == 2 * (D.OBS + D.NBLUE + 3)


def test_order_matters_within_a_lane_and_across_lanes():
    rng = np.random.default_rng(21)
    hot, cold, obs, reward, done, err, act = _random_episode(rng, 16 * 200)
    clean = D.host_digest(hot, cold, obs, reward, done, err, act)
    for which, row in ((0, hot), (1, cold)):
        for v, w in ((3, 3 + D.LANES), (70, 70 + D.LANES), (5, 6), (64 + 9, 64 + 63)):      # one lane's chain (rounds 0/1, 1/2); two lanes of round 0, of round 1
            a, b = row[16 * v:16 * v + 16].copy(), row[16 * w:16 * w + 16].copy()
            assert not np.array_equal(a, b)
            r = row.copy()
            r[16 * v:16 * v + 16], r[16 * w:16 * w + 16] = b, a
            ep = [hot, cold, obs, reward, done, err, act]
            ep[which] = r
            got = D.host_digest(*ep)
            assert got[which] != clean[which], (which, v, w)
            assert np.array_equal(got, D.digest(*ep)), (which, v, w)
    for i in (0, 7, 8, 513):
        assert obs[i] != obs[i + D.LANES]
        o = obs.copy()
        o[i], o[i + D.LANES] = obs[i + D.LANES], obs[i]
        got = D.host_digest(hot, cold, o, reward, done, err, act)
        assert got[2] != clean[2] and np.array_equal(got[:2], clean[:2]), i
        assert np.array_equal(got, D.digest(hot, cold, o, reward, done, err, act)), i
